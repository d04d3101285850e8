"""The multi-target chained tracker on search windows, on the host: the shipped config and the exports, the two
new entry points in the header, EXPORTS and the library with their argument checks (the error code before any device work), the
union-of-boxes rule, the refusals, and the dense tracker's crops at the union rectangles on a fake provider (nothing is computed)."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = ("woft_chain_tc_multi_window", "woft_mask_bbox_multi", "woft_mask_bbox_multi_ws_bytes")


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---- the config, the exports, the entry points --------------------------------------------------------------------------------------
def test_shipped_config_and_exports():
    import woft_amd
    from pytracking.tracker.WOFT_chained_multi_window import WOFTChainedMultiWindow
    from pytracking.utils.config import load_config
    from woft_amd import chained, chained_multi_window, chained_window
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained_multi_window.py")
    base = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained_multi.py")
    assert conf.tracker_class is WOFTChainedMultiWindow is chained_multi_window.WOFTChainedMultiWindow is woft_amd.WOFTChainedMultiWindow
    assert issubclass(WOFTChainedMultiWindow, chained.WOFTChainedMulti) and issubclass(WOFTChainedMultiWindow, chained_window.WOFTChainedWindow)
    assert (conf.search_window_margin, conf.flow_config.padding_mode, conf.chain_prewarp) == (0.25, "RAFT", False)
    for k in ("chain_deltas", "chain_vis_thr", "chain_unit_cost", "chain_iters", "chain_weights"):
        assert getattr(conf, k) == getattr(base, k), k
    assert conf.flow_config.raft_type == base.flow_config.raft_type and conf.flow_config.iters == base.flow_config.iters
    assert base.tracker_class is chained.WOFTChainedMulti                        # (the multi config is what it was)


def test_header_exports_and_library_agree_on_the_new_names(lib):
    from woft_amd import _lib, ops
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name), name
    assert declared == set(_lib.EXPORTS)
    assert [len(_lib._SIGS[n][1]) for n in NEW] == [20, 9, 1]
    assert all(hasattr(ops, n) for n in ("chain_tc_multi_window", "mask_bbox_multi", "mask_bbox_multi_ws"))


def _buffers(n_slots, slot_bytes=4096):
    buf = (ctypes.c_uint8 * (n_slots * slot_bytes))()
    base = ctypes.addressof(buf)
    return buf, (lambda j: base + slot_bytes * j)


def test_chain_tc_multi_window_rejects_bad_arguments_without_a_device(lib):
    """-1 before any launch (host buffers stand in for device ones: nothing is dereferenced; only refused calls are made):
    everything woft_chain_tc_multi rejects and everything the window form of woft_chain_tc_window rejects."""
    gh, gw, mh, mw, K = 5, 7, 6, 9, 3
    keep, at = _buffers(10)
    good = dict(flow=at(0), cost=at(1), vis=at(2), sel=at(3), tbits=at(4), gh=gh, gw=gw, mh=mh, mw=mw, n_targets=K, ty0=3, tx0=5,
                frame_h=40, frame_w=60, vis_thr=0.5, dst=at(5), w=at(6), ok=at(7), hist=at(8))
    order = list(good)
    call = lambda **kw: lib.woft_chain_tc_multi_window(*[dict(good, **kw)[n] for n in order], None)
    plane = 4 * gh * gw
    top = 1 << 24
    bad = [dict(flow=None), dict(cost=None), dict(vis=None), dict(sel=None), dict(tbits=None), dict(dst=None), dict(ok=None),
           dict(hist=None), dict(n_targets=0), dict(n_targets=33), dict(n_targets=-1), dict(gh=0), dict(gw=-2),
           dict(gh=top + 1), dict(mh=gh - 1), dict(mw=gw - 1), dict(vis_thr=-0.1), dict(vis_thr=1.5), dict(vis_thr=float("nan")),
           dict(dst=good["flow"]), dict(ok=good["tbits"] + 4 * mh * mw - 1), dict(w=good["dst"] + plane), dict(hist=good["sel"]),
           dict(hist=good["ok"] - 4 * 130 * K + 1), dict(hist=good["dst"] + 2 * plane - 1),
           # the window form: a negative origin, origin + side past 2^24 on either axis, a bad frame size
           dict(ty0=-1), dict(tx0=-1), dict(ty0=top - gh + 1), dict(tx0=top - gw + 1), dict(frame_h=0), dict(frame_w=0),
           dict(frame_h=-4), dict(frame_h=top + 1), dict(frame_w=top + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    del keep


def test_mask_bbox_multi_rejects_bad_arguments_without_a_device(lib):
    for n, want in ((1, 32), (5, 96), (32, 528)):
        assert lib.woft_mask_bbox_multi_ws_bytes(n) == want                      # (4 codes per target, the ticket, 3 spare ints)
    for n in (0, 33, -1):
        assert lib.woft_mask_bbox_multi_ws_bytes(n) == -1
    K = 3
    keep, at = _buffers(3)
    eye = [1.0, 0, 0, 0, 1, 0, 0, 0, 1]

    def hinv(*rows):
        return (ctypes.c_double * (9 * len(rows)))(*[v for r in rows for v in r])
    good = dict(tbits=at(0), h=6, w=9, n_targets=K, hinv=hinv(eye, eye, eye), skip=0, ws=at(1), bbox=at(2))
    order = list(good)
    call = lambda **kw: lib.woft_mask_bbox_multi(*[dict(good, **kw)[n] for n in order], None)
    nan_at_1 = [1.0, 0, 0, 0, float("nan"), 0, 0, 0, 1]
    inf_at_2 = [1.0, 0, float("inf"), 0, 1, 0, 0, 0, 1]
    bad = [dict(tbits=None), dict(hinv=None), dict(ws=None), dict(bbox=None), dict(h=0), dict(w=-1), dict(n_targets=0),
           dict(n_targets=33), dict(n_targets=-2),
           # a non-finite entry of a target that is not skipped (skipping ANOTHER target does not excuse it)
           dict(hinv=hinv(eye, nan_at_1, eye)), dict(hinv=hinv(eye, eye, inf_at_2)), dict(hinv=hinv(eye, nan_at_1, eye), skip=0b101)]
    for kw in bad:
        assert call(**kw) == -1, kw
    del keep


# ---- the union rule -----------------------------------------------------------------------------------------------------------------
def test_union_box_and_chain_rect_contain_every_targets_search_box():
    from woft_amd import window
    W, Hh = 640, 480
    boxes = [window.Box(100, 80, 60, 40), window.Box(300, 200, 50, 90), window.Box(20, 300, 30, 30)]
    u = window.union_box(boxes)
    assert u == window.Box.from_xyxy(20, 80, 349, 329) and window.union_box(boxes + [None]) == u
    assert window.union_box([boxes[0]]) == boxes[0] and window.union_box([]) is None and window.union_box([None, None]) is None
    for close in (boxes[:1], boxes[:2], boxes):
        y0, x0, rows, cols = window.chain_rect(window.union_box(close), 0.25, W, Hh, 64, 64)
        assert 0 <= y0 and 0 <= x0 and y0 + rows <= Hh and x0 + cols <= W and (rows % 64 == 0 or rows == Hh) and (cols % 64 == 0 or cols == W)
        for b in close:
            sy, sx, sr, sc = window.search_box(b, 0.25, W, Hh, 64).crop_rect()
            assert y0 <= sy and x0 <= sx and sy + sr <= y0 + rows and sx + sc <= x0 + cols, (b, (y0, x0, rows, cols))
    assert window.chain_rect(u, None, W, Hh) == (0, 0, Hh, W) == window.chain_rect(u, 0, W, Hh)


# ---- construction: keys and refusals ------------------------------------------------------------------------------------------------
class _StubProvider:
    def __init__(self, cfg):
        self.C = cfg
        self.pinned, self.bound = None, None

    def pin_source(self, img):
        self.pinned = img

    def bound_plans(self, n):
        self.bound = n


@pytest.fixture
def on_cpu(monkeypatch):
    from woft_amd import multiflow, tracker
    monkeypatch.setattr(tracker.YAOFTrackerSingleControl, "DEVICE", "cpu")
    monkeypatch.setattr(multiflow.MultiFlowTracker, "DEVICE", "cpu")
    monkeypatch.delenv("WOFT_FUSED", raising=False)


def _config(name="WOFT_chained_multi_window.py", provider=_StubProvider, **keys):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / name)
    conf.flow_config.of_class = provider
    for k, v in keys.items():
        setattr(conf, k, v)
    return conf


def test_keys_routes_and_solver_decision(on_cpu):
    from woft_amd import presets
    from woft_amd.chained_window import WOFTChainedWindow
    conf = _config()
    trk = conf.tracker_class(conf)
    assert trk._margin == 0.25 and (trk.chain_window_quantum, trk.chain_window_min, trk.chain_prewarp) == (64, 160, False)
    assert trk.flower.bound == len(trk.chain_deltas) + 1 and trk._route == "batched"
    one = WOFTChainedWindow(_config("WOFT_chained_window.py", chain_prewarp=False))
    assert trk._decision_for_meta() == one.solver_decision                       # (a target's meta names the single tracker's text)
    assert trk.solver_decision.startswith(one.solver_decision + "; multi-target planar stage")
    assert "union search window" in trk.solver_decision and "route 'batched'" in trk.solver_decision
    delattr(conf, "chain_prewarp")                                               # (absent: off here, unlike WOFTChainedWindow)
    delattr(conf, "search_window_margin")
    trk = conf.tracker_class(conf)
    assert trk.chain_prewarp is False and trk._margin is None
    for keys, route in ((dict(H_estimator=presets.estimator_ransac()), "select"), (dict(H_estimator=presets.estimator_trs()), "select"),
                        (dict(subsampler_fn=None), "loop"), (dict(device_solver=False), "loop")):
        c = _config(**keys)
        trk = c.tracker_class(c)
        assert trk._route == route and f"route '{route}'" in trk.solver_decision


@pytest.mark.parametrize("keys,exc,match", [
    (dict(chain_prewarp=True), NotImplementedError, "chain_prewarp"),
    (dict(chain_share_features=True), NotImplementedError, "chain_share_features"),
    (dict(photo_refine=True), NotImplementedError, "photo_refine"),
    (dict(visibility_mode="gate"), NotImplementedError, "visibility_mode"), (dict(fb_check="gate"), NotImplementedError, "fb_check"),
    (dict(warm_start_local=True), NotImplementedError, "warm_start_local"),
    (dict(downscale_inputs=2), NotImplementedError, "downscale_inputs"),
    (dict(post_hoc_weights_postprocessing_fn=lambda w: w), NotImplementedError, "post_hoc_weights_postprocessing_fn"),
    (dict(chain_window_quantum=12), ValueError, "quantum"), (dict(chain_deltas=(0,)), ValueError, "deltas"),
])
def test_refused_and_bad_keys_raise_at_construction(on_cpu, keys, exc, match):
    conf = _config(**keys)
    with pytest.raises(exc, match=match) as e:
        conf.tracker_class(conf)
    assert len(str(e.value)) > len(match) + 20                                 # (a reason, not only the key's name)


def test_the_refusal_reasons(on_cpu):
    from woft_amd.chained_window import WOFTChainedWindow
    conf = _config(chain_prewarp=True)
    with pytest.raises(NotImplementedError) as e:
        conf.tracker_class(conf)
    assert "one pose" in str(e.value) and "K poses" in str(e.value)
    texts = []
    for c in (_config(chain_share_features=True), _config("WOFT_chained_window.py", chain_share_features=True)):
        with pytest.raises(NotImplementedError) as e:
            c.tracker_class(c)
        texts.append(str(e.value))
    assert texts[0] == texts[1] and dict(WOFTChainedWindow.REFUSED)["chain_share_features"] in texts[0]


def test_woftchainedmulti_still_refuses_the_margin(on_cpu):
    conf = _config("WOFT_chained_multi.py", search_window_margin=0.25)
    with pytest.raises(NotImplementedError) as e:
        conf.tracker_class(conf)
    assert str(e.value) == ("search_window_margin is not provided by the chained tracker: the chains read every pixel of every "
                            "flow; the search-window tracker is WOFTWindow")


# ---- the crops of the dense tracker at the union rectangles -------------------------------------------------------------------------
FH, FW = 96, 160


class _FakeProvider:
    """Records (source crop, target crop) of every flow; frames carry (frame index, x, y) in their channels, so a crop tells its
    frame and its origin."""

    def __init__(self, cfg):
        self.C = cfg
        self.pinned, self.calls, self.bound = None, [], None

    def pin_source(self, img):
        self.pinned = img

    def bound_plans(self, n):
        self.bound = n

    def compute_flow(self, src, dst, mode=None, do_sigmoid=None, borrow=None, **kw):
        import torch
        assert mode == "flow" and do_sigmoid is False and borrow is True and src.shape == dst.shape and not kw
        ident = lambda c: (int(c[0, 0, 0]), int(c[0, 0, 2]), int(c[0, 0, 1])) + tuple(c.shape[:2])     # frame, y0, x0, rows, cols
        self.calls.append((ident(src), ident(dst)))
        return torch.zeros(2, *src.shape[:2]), None


def _frame(t):
    ys, xs = np.mgrid[:FH, :FW]
    return np.stack([np.full((FH, FW), t), xs, ys], axis=-1).astype(np.uint8)


def _box_mask(y0, x0, rows, cols):
    m = np.zeros((FH, FW), np.uint8)
    m[y0:y0 + rows, x0:x0 + cols] = 255
    return m


def test_the_provider_is_asked_for_crops_at_the_union_rectangles(on_cpu, monkeypatch):
    import torch
    from woft_amd import ops, window
    monkeypatch.setattr(ops, "crop_u8", lambda img, rect, out=None: img[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]].clone())
    boxes_seen = []

    def fake_bbox_multi(tbits, n_targets, Hmats, bbox=None, ws=None):
        """The integer translation each pose is, applied to the template boxes on the host; the launch is counted."""
        rows = []
        for t, Hm in enumerate(Hmats):
            if Hm is None:
                rows.append([0, 0, 0, 0, 0])
                continue
            dx, dy = int(round(Hm[0, 2])), int(round(Hm[1, 2]))
            y0, x0, r, c = RECTS[t]
            rows.append([y0 + dy, y0 + dy + r - 1, x0 + dx, x0 + dx + c - 1, 1])
        boxes_seen.append([Hm is not None for Hm in Hmats])
        return torch.tensor(rows, dtype=torch.int32)
    monkeypatch.setattr(ops, "mask_bbox_multi", fake_bbox_multi)
    RECTS = [(20, 16, 12, 20), (40, 60, 16, 10), (30, 30, 1, 3)]
    conf = _config(provider=_FakeProvider, chain_deltas=(None, 1, 2), chain_window_quantum=16, chain_window_min=16)
    trk = conf.tracker_class(conf)
    fold_log = []

    def fold(best, prev, flow, wl, ml, k, template_rect, step_rect, post_H, vis_thr, unit_cost, first):
        assert post_H is None and tuple(flow.shape[1:]) == tuple(step_rect[2:])
        fold_log.append((k, tuple(template_rect), tuple(step_rect)))
        h, w = template_rect[2:]
        return best or (torch.zeros(2, h, w), torch.zeros(h, w), torch.ones(h, w), torch.zeros(h, w, dtype=torch.int32))
    trk.init(_frame(0), [_box_mask(*r) for r in RECTS])
    trk.multi._fold = fold
    prov = trk.flower
    union = window.union_box([window.Box(x0, y0, c, r) for y0, x0, r, c in RECTS])
    R0 = window.chain_rect(union, 0.25, FW, FH, 16, 16)
    assert trk.chain_window == trk.multi.rect0 == R0 and R0[:2] != (0, 0) and (R0[2], R0[3]) != (FH, FW)
    assert tuple(prov.pinned.shape) == R0[2:] + (3,)
    assert tuple(trk._tbits_crop.shape) == R0[2:] and trk._tbits_crop.dtype == torch.int32
    full = trk._tbits.numpy()
    assert np.array_equal(trk._tbits_crop.numpy(), full[R0[0]:R0[0] + R0[2], R0[1]:R0[1] + R0[3]])
    assert sorted(np.unique(full).tolist()) == [0, 1, 2, 5]                      # (the 1 x 3 mask lies inside mask 0: bits 0 and 2)
    assert [T._template_box for T in trk._targets] == [window.Box(x0, y0, c, r) for y0, x0, r, c in RECTS]

    def shift(dx, dy):                                                           # cur -> init of a target that moved by (dx, dy)
        return np.array([[1.0, 0, -dx], [0, 1, -dy], [0, 0, 1]])
    # per frame the poses of the three targets (None: singular): frame 1 all identity (no launch), frame 2 two moved and one
    # still at its template box, frame 3 one singular, frame 4 nobody contributes (the window stays)
    singular = np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]])
    poses = {1: [np.eye(3)] * 3, 2: [shift(24, 8), np.eye(3), shift(8, 0)], 3: [shift(40, 16), singular, shift(16, 0)],
             4: [singular, np.full((3, 3), np.nan), singular]}
    moved = lambda t, d: window.Box(RECTS[t][1] + d[0], RECTS[t][0] + d[1], RECTS[t][3], RECTS[t][2])
    want_boxes = {1: [moved(0, (0, 0)), moved(1, (0, 0)), moved(2, (0, 0))], 2: [moved(0, (24, 8)), moved(1, (0, 0)), moved(2, (8, 0))],
                  3: [moved(0, (40, 16)), None, moved(2, (16, 0))]}
    rects = {0: R0}
    for f in (1, 2, 3, 4, 5):
        del prov.calls[:], fold_log[:]
        out = trk.multi.track(_frame(f))
        assert out.rect == R0
        sched = trk.multi.schedule(f)
        want = [((s,) + (rects[s] if chained else R0), (f,) + (rects[s] if chained else R0)) for _, s, chained in sched]
        assert prov.calls == want, (f, prov.calls, want)
        assert fold_log == [(k, R0, rects[s] if chained else R0) for k, s, chained in sched]
        if f == 5:
            break
        for T, P in zip(trk._targets, poses[f]):
            T.prev_H2init = P
        n_launch = len(boxes_seen)
        trk._follow()
        if f in want_boxes:
            rects[f] = window.chain_rect(window.union_box(want_boxes[f]), 0.25, FW, FH, 16, 16)
        else:
            rects[f] = rects[f - 1]                                              # (no contributor: the previous window)
        assert trk.chain_window == rects[f], (f, trk.chain_window, rects[f])
        assert len(boxes_seen) - n_launch == (0 if f in (1, 4) else 1)          # (all identity / nobody finite: no launch)
        # the ring holds crops by their rectangles and results on R0
        for s, (crop, rect, res) in trk.multi._ring.items():
            assert rect == rects[s] and tuple(crop.shape[:2]) == rect[2:] and tuple(res[0].shape) == (2,) + R0[2:]
    assert boxes_seen == [[True, False, True], [True, False, True]]              # (identity and singular poses are skipped)
    assert len(set(rects.values())) >= 3
