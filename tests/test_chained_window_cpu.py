"""WOFTChainedWindow and WindowedMultiFlowTracker on the host: the shipped config and the exports, the config
keys (the window class accepts `search_window_margin`, WOFTChained still refuses it with its present text), and the dense tracker's
schedule of crops, rectangles and ring entries on a fake provider and a fake fold (nothing is computed)."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


class _StubProvider:
    """Has what the chained tracker asks of a provider; a 'flow' is a zero map."""

    def __init__(self, cfg):
        self.C = cfg
        self.pinned, self.bound = None, None

    def pin_source(self, img):
        self.pinned = img

    def bound_plans(self, n):
        self.bound = n

    def compute_flow(self, src, dst, mode=None, do_sigmoid=None, borrow=None, **kw):
        import torch
        assert mode == "flow" and do_sigmoid is False and borrow is True
        return torch.zeros(2, *src.shape[:2]), None


@pytest.fixture
def on_cpu(monkeypatch):
    from woft_amd import multiflow, tracker
    monkeypatch.setattr(tracker.YAOFTrackerSingleControl, "DEVICE", "cpu")
    monkeypatch.setattr(multiflow.MultiFlowTracker, "DEVICE", "cpu")
    monkeypatch.delenv("WOFT_FUSED", raising=False)


def _config(name="WOFT_chained_window.py", **keys):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / name)
    conf.flow_config.of_class = _StubProvider
    for k, v in keys.items():
        setattr(conf, k, v)
    return conf


def test_shipped_config_and_exports():
    import woft_amd
    from pytracking.tracker.WOFT_chained_window import WOFTChainedWindow
    from pytracking.utils.config import load_config
    from woft_amd import chained, chained_window, window
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained_window.py")
    base = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained.py")
    assert conf.tracker_class is WOFTChainedWindow is chained_window.WOFTChainedWindow is woft_amd.WOFTChainedWindow
    assert issubclass(WOFTChainedWindow, chained.WOFTChained)
    assert (conf.search_window_margin, conf.chain_window_quantum, conf.chain_window_min, conf.chain_prewarp) \
        == (0.25, 64, window.MIN_WINDOW, True)
    assert conf.flow_config.padding_mode == "RAFT" and tuple(conf.chain_deltas) == tuple(base.chain_deltas)
    assert conf.flow_config.raft_type == base.flow_config.raft_type and conf.flow_config.iters == base.flow_config.iters
    # the demo loads a config by its path and builds config.tracker_class: nothing there names a tracker
    demo = (ROOT / "tools" / "woft_demo_headless.py").read_text()
    assert "load_config(config_path)" in demo and "config.tracker_class(config)" in demo
    assert "WOFT_chained_window" in (ROOT / "INTEGRATION.md").read_text()


def test_the_window_class_accepts_the_margin_and_woftchained_still_refuses_it(on_cpu):
    from woft_amd.chained import WOFTChained
    conf = _config()
    trk = conf.tracker_class(conf)
    assert trk._margin == 0.25 and (trk.chain_window_quantum, trk.chain_window_min, trk.chain_prewarp) == (64, 160, True)
    assert trk.flower.bound == len(trk.chain_deltas) + 1
    assert "search windows" in trk.solver_decision and "margin 0.25" in trk.solver_decision
    for k in ("search_window_margin", "chain_window_quantum", "chain_window_min", "chain_prewarp"):
        delattr(conf, k)                                                       # (every window key is optional)
    trk = conf.tracker_class(conf)
    assert trk._margin is None and (trk.chain_window_quantum, trk.chain_window_min, trk.chain_prewarp) == (64, 160, True)
    conf = _config("WOFT_chained.py", search_window_margin=0.25)
    with pytest.raises(NotImplementedError) as e:
        WOFTChained(conf)
    assert str(e.value) == ("search_window_margin is not provided by the chained tracker: the chains read every pixel of every "
                            "flow; the search-window tracker is WOFTWindow")


@pytest.mark.parametrize("keys,exc,match", [
    (dict(chain_share_features=True), NotImplementedError, "chain_share_features"),
    (dict(visibility_mode="gate"), NotImplementedError, "visibility_mode"), (dict(fb_check="gate"), NotImplementedError, "fb_check"),
    (dict(downscale_inputs=2), NotImplementedError, "downscale_inputs"),
    (dict(chain_window_quantum=12), ValueError, "quantum"), (dict(chain_window_quantum=0), ValueError, "quantum"),
    (dict(chain_deltas=(0,)), ValueError, "deltas"),
])
def test_refused_and_bad_keys_raise_at_construction(on_cpu, keys, exc, match):
    conf = _config(**keys)
    with pytest.raises(exc, match=match) as e:
        conf.tracker_class(conf)
    assert len(str(e.value)) > len(match) + 20                                 # (a reason, not only the key's name)


# ---- the dense tracker's schedule of crops -------------------------------------------------------------------------------------
class _FakeProvider:
    """Records (source crop, target crop) of every flow; frames carry (frame index, x, y) in their channels, so a crop tells its
    frame and its origin."""

    def __init__(self):
        self.C = SimpleNamespace()
        self.pinned, self.calls, self.bound = None, [], None

    def pin_source(self, img):
        self.pinned = img

    def bound_plans(self, n):
        self.bound = n

    def compute_flow(self, src, dst, mode=None, do_sigmoid=None, borrow=None, **kw):
        import torch
        assert mode == "flow" and do_sigmoid is False and borrow is True and src.shape == dst.shape
        ident = lambda c: (int(c[0, 0, 0]), int(c[0, 0, 2]), int(c[0, 0, 1])) + tuple(c.shape[:2])     # frame, y0, x0, rows, cols
        self.calls.append((ident(src), ident(dst), src is self.pinned, kw))
        return torch.zeros(2, *src.shape[:2]), None


def _frame(t, h=40, w=60):
    ys, xs = np.mgrid[:h, :w]
    return np.stack([np.full((h, w), t), xs, ys], axis=-1).astype(np.uint8)


def _fake_tracker(monkeypatch, **kw):
    import torch
    from woft_amd import chained_window, multiflow, ops
    monkeypatch.setattr(multiflow.MultiFlowTracker, "DEVICE", "cpu")
    monkeypatch.setattr(ops, "crop_u8", lambda img, rect, out=None: img[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]].clone())
    prov = _FakeProvider()
    trk = chained_window.WindowedMultiFlowTracker(prov, **kw)
    log = []

    def fold(best, prev, flow, wl, ml, k, template_rect, step_rect, post_H, vis_thr, unit_cost, first):
        assert first == (best is None) and tuple(flow.shape[1:]) == tuple(step_rect[2:])
        assert prev is None or tuple(prev[0].shape[1:]) == tuple(template_rect[2:])
        log.append((k, tuple(template_rect), tuple(step_rect), prev is not None, post_H is not None))
        h, w = template_rect[2:]
        return best or (torch.zeros(2, h, w), torch.zeros(h, w), torch.ones(h, w), torch.zeros(h, w, dtype=torch.int32))
    trk._fold = fold
    return trk, prov, log


def test_crops_rectangles_and_ring_of_the_windowed_dense_tracker(monkeypatch):
    trk, prov, log = _fake_tracker(monkeypatch, deltas=(None, 1, 2))
    assert prov.bound == 4 and trk.share_features is False
    with pytest.raises(TypeError, match="share_features"):                     # (not offered: the crops of a frame differ per flow)
        type(trk)(prov, share_features=True)
    R0 = (4, 8, 16, 24)
    with pytest.raises(RuntimeError, match="init"):
        trk.track(_frame(1))
    with pytest.raises(ValueError, match="leaves"):
        trk.init(_frame(0), (30, 8, 16, 24))
    trk.init(_frame(0), R0)
    assert tuple(prov.pinned.shape) == (16, 24, 3) and trk.rect0 == R0
    rects = {0: R0, 1: (6, 10, 16, 32), 2: (0, 0, 40, 60), 3: (20, 30, 8, 16)}
    for t in (1, 2, 3, 4):
        del log[:], prov.calls[:]
        out = trk.track(_frame(t))
        assert out.rect == R0 and tuple(out.flow.shape) == (2, 16, 24) and tuple(out.sel.shape) == (1, 16, 24) and out.frame_index == t
        sched = trk.schedule(t)
        assert [c[0] for c in log] == [k for k, _, _ in sched]
        for (k, s, chained), (src, dst, pinned, kw), (_, trect, srect, has_prev, has_post) in zip(sched, prov.calls, log):
            B = rects[s] if chained else R0
            assert src == (s,) + B and dst == (t,) + B and kw == {}           # (the stored crop of frame s, the same rect of frame t)
            assert trect == R0 and srect == B and has_prev == chained and not has_post
            assert pinned == (not chained or (s == 0 and B == R0))
        if t in rects:
            trk.set_rect(rects[t])
            with pytest.raises(RuntimeError, match="already"):
                trk.set_rect(rects[t])
        # the ring: crops by their rects and results on R0; nothing whole-frame but the frame whose rect is the whole frame
        for s, (crop, rect, res) in trk._ring.items():
            assert tuple(crop.shape[:2]) == rect[2:] and tuple(res[0].shape) == (2, 16, 24) and tuple(res[1].shape) == (16, 24)
        if t in rects:
            assert sorted(trk._ring) == list(range(max(0, t - 1), t + 1)) and trk._pending is None, t
        else:                                                                  # (held whole until its rect is known: R0 at the next track())
            assert sorted(trk._ring) == [t - 2, t - 1] and trk._pending[0] == t
    rects[4] = R0
    del log[:], prov.calls[:]
    trk.track(_frame(5))
    assert [(src, dst) for src, dst, _, _ in prov.calls] == [((0,) + R0, (5,) + R0), ((4,) + R0, (5,) + R0), ((3,) + rects[3], (5,) + rects[3])]
    assert sorted(trk._ring) == [3, 4]
    with pytest.raises(ValueError, match="frame"):
        trk.track(_frame(5, 41, 60))
    trk.reset()
    assert trk._ring == {} and trk._template is None and trk.rect0 is None


def test_prewarp_reaches_the_direct_candidate_only(monkeypatch):
    from woft_amd import ops
    trk, prov, log = _fake_tracker(monkeypatch, deltas=(None, 1))
    warped = []
    monkeypatch.setattr(ops, "warp_perspective_window_u8",
                        lambda img, Hm, rect, out=None, valid=None, nearest=False: (warped.append((tuple(rect), np.array(Hm))),
                                                                                    out.copy_(img[:rect[2], :rect[3]])))
    R0 = (4, 8, 16, 24)
    trk.init(_frame(0), R0)
    trk.track(_frame(1), prewarp_H=np.eye(3))
    assert warped == [] and [c[4] for c in log] == [False, False]
    del log[:]
    Hm = np.array([[1, 0, 3.0], [0, 1, -2.0], [0, 0, 1]])
    trk.track(_frame(2), prewarp_H=Hm)
    assert len(warped) == 1 and warped[0][0] == R0 and np.array_equal(warped[0][1], Hm)
    assert [(c[0], c[3], c[4]) for c in log] == [(0, False, True), (1, True, False)]
