"""The multi-target chained tracker on search windows, on the GPU.  Every expected value comes from an existing
entry point or tracker: woft_chain_tc_multi_window against K woft_chain_tc_window calls (and woft_chain_tc_multi where the gate
cannot bite), woft_mask_bbox_multi against K woft_mask_bbox calls, WOFTChainedMultiWindow with one mask against WOFTChainedWindow,
with whole-frame windows against WOFTChainedMulti, its batched routes against its own loop of the single-target stage, a known
motion of three targets on a stub provider, the launches and reads of a track() (which must not depend on K), the plans the
provider keeps, and the window's fall-back."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import chained_multi_util as U  # noqa: E402
import test_chained_window_gpu as W  # noqa: E402  (its helpers: flow configs, stub frames; nothing of it is edited)
from launch_trace import d2h_copies  # noqa: E402
from woft_amd import _lib, ops, presets, synth, window  # noqa: E402
from woft_amd.chained import pack_target_bits  # noqa: E402

cuda = W.cuda


def tbits_of(masks):
    return cuda(pack_target_bits(masks).view(np.int32))


def u8(m):
    return cuda((np.asarray(m) != 0).astype(np.uint8) * 255)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. woft_chain_tc_multi_window --------------------------------------------------------------------------------------------------
RECTS = [(40, 56, None), (37, 70, (41, 75))]             # (gh, gw, size of the cropped masks: None = the grid's); 70 is no multiple of 64


@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("origin", [(0, 0), (3, 5)])
@pytest.mark.parametrize("rect", RECTS)
def test_chain_tc_multi_window_equals_k_window_calls(rect, origin, K):
    gh, gw, mask_hw = rect
    mh, mw = mask_hw or (gh, gw)
    ty0, tx0 = origin
    frame_hw = (ty0 + gh - 6, tx0 + gw - 10)              # (the rectangle's last 6 rows and 10 columns lie outside the frame)
    c = U.make_fold(gh, gw, seed=gh + K)
    masks = U.make_masks(mh, mw, K, seed=K)
    dev = {k: cuda(v) for k, v in c.items()}
    args = (dev["flow"], dev["cost"], dev["vis"], dev["sel"])
    tb = tbits_of(masks)
    for want_w in (True, False):
        dst, w, ok, hist = ops.chain_tc_multi_window(*args, tb, K, 0.5, origin, frame_hw, want_w=want_w, mask_hw=(mh, mw))
        again = ops.chain_tc_multi_window(*args, tb, K, 0.5, origin, frame_hw, want_w=want_w, mask_hw=(mh, mw))
        assert (w is None) == (not want_w) and tuple(hist.shape) == (K, ops.CHAIN_HIST)
        for a, b in zip((dst, w, ok, hist), again):                              # (two calls: equal bytes)
            assert a is None or same_bits(a, b)
        for t in range(K):
            d1, w1, ok1, h1 = ops.chain_tc_window(*args, u8(masks[t]), 0.5, origin, frame_hw, want_w=want_w, mask_hw=(mh, mw))
            assert same_bits(dst, d1) and same_bits(ok, ok1) and (w is None or same_bits(w, w1)), t
            assert torch.equal(hist[t], h1), (t, hist[t].nonzero().flatten().tolist(), h1.nonzero().flatten().tolist())
            assert int(h1.sum()) == int((masks[t][:gh, :gw] != 0).sum())
    # the gate is exercised: a real share of the landings that pass the plain rule leaves the frame
    _, _, ok_plain, _ = ops.chain_tc(*args, None, 0.5)
    share = 1.0 - float(ok.sum()) / float(ok_plain.sum())
    print(f"rect {gh} x {gw} at {origin}, frame {frame_hw}: {share:.3f} of the visible landings leave the frame")
    assert 0.1 < share < 0.9, share
    # ... and the histograms do not follow the gate: they are woft_chain_tc_multi's
    _, _, _, hist_plain = ops.chain_tc_multi(*args, tb, K, 0.5, mask_hw=(mh, mw))
    assert torch.equal(hist, hist_plain)


@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("rect", RECTS)
def test_chain_tc_multi_window_in_a_frame_that_holds_every_landing_is_chain_tc_multi(rect, K):
    gh, gw, mask_hw = rect
    mh, mw = mask_hw or (gh, gw)
    c = U.make_fold(gh, gw, seed=3 * gh + K)
    c["flow"] = np.abs(c["flow"])                         # (no landing left of or above the origin; NaN stays NaN)
    dev = {k: cuda(v) for k, v in c.items()}
    args = (dev["flow"], dev["cost"], dev["vis"], dev["sel"])
    tb = tbits_of(U.make_masks(mh, mw, K, seed=K))
    got = ops.chain_tc_multi_window(*args, tb, K, 0.5, (0, 0), (4096, 4096), mask_hw=(mh, mw))
    want = ops.chain_tc_multi(*args, tb, K, 0.5, mask_hw=(mh, mw))
    for name, a, b in zip(("dst", "w", "ok", "hist"), got, want):
        assert same_bits(a, b), name
    assert bool(torch.isnan(got[0]).any()) and 0 < float(got[2].sum()) < gh * gw


# ---- 2. woft_mask_bbox_multi --------------------------------------------------------------------------------------------------------
BH, BW = 64, 80


def _poses():
    """mask -> frame: one whose vanishing line (x = 40) crosses the mask it carries (mask 0 holds columns 20 .. 59), a general
    homography, one that moves a mask partly out of the frame, one fully out, the identity."""
    a = np.deg2rad(7.0)
    general = np.array([[1.05 * np.cos(a), -np.sin(a), 6.3], [np.sin(a), 0.95 * np.cos(a), -4.6], [4e-4, -3e-4, 1.0]])
    partly = np.array([[1.0, 0.02, 47.4], [-0.01, 1.0, -20.7], [0, 0, 1.0]])
    out = np.array([[1.0, 0, 900.5], [0, 1.0, 0], [0, 0, 1.0]])
    vanishing = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1.0 / 40.0, 0, 1.0]])
    return [vanishing, general, partly, out, np.eye(3)]


@pytest.mark.parametrize("K", [1, 5, 32])
def test_mask_bbox_multi_equals_k_single_calls(K):
    masks = U.make_masks(BH, BW, K, seed=K)
    if K >= 3:
        assert not masks[1].any() and masks[2].all() and (masks[0] & masks[2]).any()
    poses = _poses()
    rng = np.random.default_rng(K)
    Hs = []
    for t in range(K):
        Hm = poses[(t + 1) % 5 if K == 1 else t % 5].copy()                       # (K = 1: the general homography)
        if t >= 5:                                                               # (further targets: the five poses, jittered)
            Hm[:2, 2] += rng.uniform(-3, 3, 2)
        Hs.append(Hm)
    tb = tbits_of(masks)
    ws = torch.zeros(int(_lib.load().woft_mask_bbox_multi_ws_bytes(K)), dtype=torch.uint8, device="cuda")
    got = ops.mask_bbox_multi(tb, K, Hs, ws=ws)
    again = ops.mask_bbox_multi(tb, K, Hs, ws=ws)
    assert got.dtype == torch.int32 and tuple(got.shape) == (K, 5) and torch.equal(got, again)
    assert not bool(ws.any())                                                    # (left zeroed)
    want = torch.stack([ops.mask_bbox(u8(masks[t]), Hmat=Hs[t]) for t in range(K)])
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    rows = got.tolist()
    print(f"K = {K}: {rows[:5]}")
    if K >= 5:
        assert rows[1] == [0, 0, 0, 0, 0] and rows[3] == [0, 0, 0, 0, 0]         # the empty mask; the mask carried fully out
        assert rows[0][4] == 1 and masks[0][:, 20:60].any() and masks[3].any()  # carried across its vanishing line: still measured
        assert rows[4][4] == 1                                                   # the identity
        assert rows[2][4] == 1 and rows[2][0] == 0 and rows[2][3] == BW - 1      # the full mask partly out: cut at the frame's edges
    # skipped targets: rows of zeros, the others unchanged; a skipped target's matrix is never read
    skipped = [None if t % 2 == 0 else Hm for t, Hm in enumerate(Hs)]
    part = ops.mask_bbox_multi(tb, K, skipped, ws=ws)
    for t in range(K):
        assert part[t].tolist() == ([0, 0, 0, 0, 0] if t % 2 == 0 else rows[t]), t
    assert not bool(ws.any())


# ---- a stub provider with two motions -----------------------------------------------------------------------------------------------
SH, SW, S_FRAMES, S_DELTAS = W.SH, W.SW, W.S_FRAMES, W.S_DELTAS                   # 96 x 128 frames, six of them, (None, 1, 2, 4)
BOUND_PX = W.BOUND_PX                                                             # 1e-2 px: test_chained_window_gpu.py's bound
SPLIT = 61                                                                        # template column: left of it motion a, else motion b
MASK_A, MASK_B, MASK_C = (30, 30, 20, 24), (44, 70, 16, 20), (25, 40, 1, 3)       # (y0, x0, rows, cols); c: three pixels, on a's side


def _motion(label, t):
    """Frame 0 -> frame t of the plane `label`: a small rotation and anisotropic scale about the plane's centre and a translation,
    a towards the top left, b towards the bottom right."""
    sign, centre, step = {"a": (1.0, np.array([41.5, 39.5]), np.array([-2.2, -1.4])),
                          "b": (-1.0, np.array([79.5, 51.5]), np.array([3.2, 1.8]))}[label]
    c, s = np.cos(0.008 * sign * t), np.sin(0.008 * sign * t)
    L = np.array([[c, -s], [s, c]]) @ np.diag([1 + 0.003 * t, 1 - 0.002 * t])
    A = np.eye(3)
    A[:2, :2], A[:2, 2] = L, centre - L @ centre + step * t
    return A


class _TwoMotionProvider:
    """Analytic flows on crops, in the style of test_chained_window_gpu._MotionProvider.  Frames carry (frame index, x, y) in their
    channels, so a crop tells its frame and its origin.  A pixel of frame s belongs to plane a when motion a takes it back to a
    template column left of SPLIT, else to plane b (the planes move apart: no pixel of either mask changes sides).  The first call
    of every frame is the direct candidate: 5 px off with reliability logit -4; the chained flows are exact with +4."""
    precision, precision_source = "stub", "stub"

    def __init__(self, cfg):
        self.C, self.pinned, self.calls, self._last_t, self.bound = cfg, None, [], None, None

    def pin_source(self, img):
        self.pinned = img

    def bound_plans(self, n):
        self.bound = n

    def compute_flow(self, src, dst, mode=None, do_sigmoid=None, borrow=None, **kw):
        assert mode == "flow" and do_sigmoid is False and borrow is True and not kw and src.shape == dst.shape
        head = torch.stack([src[0, 0], dst[0, 0]]).cpu().numpy()                  # (one read: frame index, x, y of both corners)
        s, x0, y0 = (int(v) for v in head[0])
        t = int(head[1, 0])
        assert (int(head[1, 1]), int(head[1, 2])) == (x0, y0)                    # (the same rect of both frames)
        rows, cols = src.shape[:2]
        direct, self._last_t = t != self._last_t, t
        self.calls.append((s, t, (y0, x0, rows, cols), direct))
        ys, xs = np.mgrid[y0:y0 + rows, x0:x0 + cols].astype(np.float64)
        flows = {}
        for label in "ab":
            M = _motion(label, t) @ np.linalg.inv(_motion(label, s))
            flows[label] = np.stack([M[0, 0] * xs + M[0, 1] * ys + M[0, 2] - xs, M[1, 0] * xs + M[1, 1] * ys + M[1, 2] - ys])
        back = np.linalg.inv(_motion("a", s))
        is_a = back[0, 0] * xs + back[0, 1] * ys + back[0, 2] < SPLIT
        flow = np.where(is_a[None], flows["a"], flows["b"])
        if direct:
            flow = flow + np.array([3.0, 4.0])[:, None, None]
        return cuda(flow.astype(np.float32)), torch.full((1, rows, cols), -4.0 if direct else 4.0, device="cuda")


def _rect_mask(rect):
    m = np.zeros((SH, SW), np.uint8)
    m[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]] = 255
    return m


def _two_motion_tracker(masks, estimator=None, route=None, **keys):
    from pytracking.utils.config import load_config
    conf = load_config(U.ROOT / "pytracking" / "configs" / "WOFT_chained_multi_window.py")
    conf.flow_config.of_class = _TwoMotionProvider
    conf.chain_deltas, conf.chain_window_min, conf.chain_window_quantum = S_DELTAS, 32, 16
    if estimator is not None:
        conf.H_estimator = estimator
    for k, v in keys.items():
        setattr(conf, k, v)
    trk = conf.tracker_class(conf)
    if route is not None:
        trk._route = route                                                       # (forced before init(): the loop needs its mask crops)
    trk.init(W._stub_frame(0), masks)
    return trk


def _assert_same_frames(res_a, res_b, tag):
    """[(Hs, metas)] per frame of two runs: equal bytes, every meta field."""
    assert len(res_a) == len(res_b)
    for f, ((Ha, ma), (Hb, mb)) in enumerate(zip(res_a, res_b), 1):
        assert Ha.dtype == Hb.dtype == np.float64 and np.array_equal(Ha, Hb), (tag, f, Ha, Hb)
        for t, (a, b) in enumerate(zip(ma, mb)):
            a, b = vars(a), vars(b)
            assert sorted(a) == sorted(b), (tag, f, t)
            for k in a:
                assert U.same_value(a[k], b[k]), (tag, k, f, t, a[k], b[k])


# ---- 3. one mask: WOFTChainedWindow, byte for byte ------------------------------------------------------------------------------------
def _single_vs_multi(make, frames, frame0, mask):
    """-> ([(H, meta)] of WOFTChainedWindow, [(Hs, metas)] of the new tracker with the one mask), built by make(config name)."""
    one = make("WOFT_chained_window.py")
    one.init(frame0, mask)
    single = [one.track(f) for f in frames]
    trk = make("WOFT_chained_multi_window.py")
    trk.init(frame0, [mask])
    multi = [trk.track(f) for f in frames]
    assert trk.multi.rect0 == one.multi.rect0 and trk.multi.rect0[2:] != tuple(frame0.shape[:2])      # (a window, not the frame)
    return one, trk, single, multi


def _check_single_vs_multi(single, multi, tag):
    for f, ((H1, m1), (Hs, metas)) in enumerate(zip(single, multi), 1):
        assert Hs.shape == (1, 3, 3) and Hs.dtype == np.float64 and np.array_equal(Hs[0], H1), (tag, f, Hs[0], H1)
        a, b = vars(metas[0]), vars(m1)
        assert sorted(a) == sorted(b), (tag, f, sorted(a), sorted(b))
        for k in a:
            assert U.same_value(a[k], b[k]), (tag, k, f, a[k], b[k])


@pytest.mark.parametrize("fused", [True, False])
def test_one_mask_on_the_stub_provider_returns_woftchainedwindows_bytes(monkeypatch, fused):
    monkeypatch.setenv("WOFT_FUSED", "1" if fused else "0")
    from pytracking.utils.config import load_config

    def make(name):
        conf = load_config(U.ROOT / "pytracking" / "configs" / name)
        conf.flow_config.of_class = lambda fc: W._MotionProvider(fc, "direct")
        conf.chain_deltas, conf.chain_window_min, conf.chain_window_quantum, conf.chain_prewarp = S_DELTAS, 32, 16, False
        trk = conf.tracker_class(conf)
        trk.flower.tracker = trk
        assert (trk._fused is not None) == fused
        return trk
    one, trk, single, multi = _single_vs_multi(make, [W._stub_frame(t) for t in range(1, S_FRAMES + 1)], W._stub_frame(0), W._stub_mask())
    assert trk._route == ("batched" if fused else "loop")
    _check_single_vs_multi(single, multi, f"stub fused={fused}")
    assert trk.flower.calls == one.flower.calls and trk.chain_window == one.chain_window != trk.multi.rect0
    assert not any(m.lost for _, m in single)


@pytest.mark.parametrize("fused", [True, False])
def test_one_mask_on_the_real_provider_returns_woftchainedwindows_bytes(monkeypatch, fused):
    monkeypatch.setenv("WOFT_FUSED", "1" if fused else "0")
    Hh, Ww = 128, 160
    template = synth.make_template(Hh, Ww, seq_id=3)
    frames = [synth.make_frame(template, t) for t in range(1, 7)]

    def make(name):
        conf = W._tracker_config(name, "weighted", chain_deltas=(None, 1, 2), chain_prewarp=False, chain_window_min=64,
                                 chain_window_quantum=32)
        trk = conf.tracker_class(conf)
        assert (trk._fused is not None) == fused
        return trk
    one, trk, single, multi = _single_vs_multi(make, frames, template, synth.make_init_mask(Hh, Ww))
    _check_single_vs_multi(single, multi, f"real fused={fused}")
    assert any(not np.array_equal(H1, np.eye(3)) and np.isfinite(H1).all() for H1, _ in single)


# ---- 4. a falsy margin: WOFTChainedMulti, byte for byte -----------------------------------------------------------------------------
def test_whole_frame_windows_return_woftchainedmultis_bytes(monkeypatch):
    from woft_amd import WOFTChainedMultiWindow
    monkeypatch.setenv("WOFT_FUSED", "1")
    frame0, frames = U.stub_frames()
    masks = U.stub_masks()
    conf = U.stub_config(True)
    ref = conf.tracker_class(conf)
    ref.init(frame0, masks)
    want = [ref.track(f) for f in frames]
    conf = U.stub_config(True)
    conf.tracker_class, conf.search_window_margin = WOFTChainedMultiWindow, None
    trk = conf.tracker_class(conf)
    assert trk._route == ref._route == "batched"
    trk.init(frame0, masks)
    got = [trk.track(f) for f in frames]
    assert trk.chain_window == trk.multi.rect0 == (0, 0, U.SH, U.SW)
    # what the window class adds to a meta: the window, and its own clause of the (first frame's) solver text
    for (_, metas), (_, ref_metas) in zip(got, want):
        for m, r in zip(metas, ref_metas):
            assert m.chain_window == (0, 0, U.SH, U.SW)
            del m.chain_window
            if hasattr(r, "solver_decision"):
                assert m.solver_decision.startswith(r.solver_decision) and "search windows" in m.solver_decision
                m.solver_decision = r.solver_decision
    K = len(masks)
    U.assert_same_result(got, [[(Hs[t], metas[t]) for Hs, metas in want] for t in range(K)], "whole frame")
    assert not want[-1][1][0].lost and want[-1][1][2].lost


# ---- 5. the batched routes equal the loop route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator,route", [(None, "batched"), (presets.estimator_ransac(10000, 3.0, 0.995), "select")])
def test_the_batched_routes_equal_the_loop_of_the_single_target_stage(monkeypatch, estimator, route):
    monkeypatch.setenv("WOFT_FUSED", "1")
    masks = [_rect_mask(MASK_A), _rect_mask(MASK_B)]
    frames = [W._stub_frame(t) for t in range(1, S_FRAMES + 1)]
    trk = _two_motion_tracker(masks, estimator)
    assert trk._route == route
    got = [trk.track(f) for f in frames]
    loop = _two_motion_tracker(masks, estimator, route="loop")
    want = [loop.track(f) for f in frames]
    _assert_same_frames(got, want, route)
    wins = [metas[0].chain_window for _, metas in got]
    assert len(set(wins)) >= 2 and all(w[2] < SH or w[3] < SW for w in wins) and trk.multi.rect0[:2] != (0, 0)
    assert not any(m.lost for _, metas in got for m in metas) and trk.flower.calls == loop.flower.calls
    assert not np.array_equal(got[-1][0][0], got[-1][0][1])                      # (two poses: the targets move apart)


# ---- 6. a known motion ----------------------------------------------------------------------------------------------------------------
def _corner_error(Hm, rect, label, t):
    y0, x0, rows, cols = rect
    c = np.array([[x0, y0, 1], [x0 + cols - 1, y0, 1], [x0 + cols - 1, y0 + rows - 1, 1], [x0, y0 + rows - 1, 1.0]]).T
    a, b = Hm @ c, np.linalg.inv(_motion(label, t)) @ c
    return float(np.abs(a[:2] / a[2] - b[:2] / b[2]).max())


def test_known_motion_of_three_targets_on_one_union_window(monkeypatch):
    monkeypatch.setenv("WOFT_FUSED", "1")
    rects_in = [MASK_A, MASK_B, MASK_C]
    masks = [_rect_mask(r) for r in rects_in]
    trk = _two_motion_tracker(masks)
    chain = lambda box: window.chain_rect(box, 0.25, SW, SH, 16, 32)
    tboxes = [window.Box(r[1], r[0], r[3], r[2]) for r in rects_in]
    R0 = chain(window.union_box(tboxes))
    assert trk.multi.rect0 == trk.chain_window == R0 and R0[:2] != (0, 0) and trk.flower.bound == len(S_DELTAS) + 1
    rects, errs = {0: R0}, []
    for t in range(1, S_FRAMES + 1):
        Hs, metas = trk.track(W._stub_frame(t))
        # the true carried boxes, by the existing single-mask entry point on the true motion; the lost target keeps the identity
        true = []
        for label, m in (("a", masks[0]), ("b", masks[1])):
            rmin, rmax, cmin, cmax, any_set = ops.mask_bbox(u8(m), Hmat=_motion(label, t)).cpu().tolist()
            assert any_set
            true.append(window.Box.from_extent(rmin, rmax, cmin, cmax))
        rects[t] = chain(window.union_box(true + [tboxes[2]]))
        assert all(m.chain_window == rects[t] for m in metas) and trk.chain_window == rects[t], (t, metas[0].chain_window, rects[t])
        for k, (label, rect) in enumerate((("a", MASK_A), ("b", MASK_B))):
            assert not metas[k].lost and metas[k].global_H_success and metas[k].n_kept == rect[2] * rect[3]
            errs.append(_corner_error(Hs[k], rect, label, t))
            print(f"frame {t} target {label}: window {metas[k].chain_window}, kept {metas[k].n_kept}, corner error {errs[-1]:.2e} px")
            assert errs[-1] <= BOUND_PX, (t, label, errs[-1])
            assert metas[k].chain_hist.sum() + metas[k].chain_invalid + metas[k].chain_occluded == rect[2] * rect[3]
        # three pixels never make four correspondences: lost on every frame, its pose the identity, nobody else disturbed
        assert metas[2].lost and metas[2].N_lost == t and metas[2].n_kept <= 3 and metas[2].H_global_cur2init is None
        assert np.array_equal(Hs[2], np.eye(3))
    assert len(set(rects.values())) >= 3 and rects[S_FRAMES] != R0
    want = [(s, t, R0 if not chained else rects[s], not chained)
            for t in range(1, S_FRAMES + 1) for _, s, chained in trk.multi.schedule(t)]
    assert trk.flower.calls == want
    print(f"known motion, frames 1..{S_FRAMES}: largest corner error {max(errs):.2e} px (bound {BOUND_PX} px)")


# ---- 7. launches and reads do not depend on K -----------------------------------------------------------------------------------------
def _trace_one_track(K):
    masks = [_rect_mask((22 + t, 24 + t, 20, 24)) for t in range(K)]              # (all on plane a: columns below SPLIT)
    trk = _two_motion_tracker(masks)
    trk.track(W._stub_frame(1))                                                  # (buffers allocated, library loaded, poses no longer the identity)
    copies = []
    with pytest.MonkeyPatch.context() as patch:
        proxy = U.CountingLib(_lib.load())
        patch.setattr(_lib, "_lib", proxy)
        d2h_copies(patch, copies.append)
        real = trk.flower.compute_flow

        def unseen(*a, **kw):                                                    # (the stub's own read of the crops' corners is not the tracker's)
            before = len(copies)
            out = real(*a, **kw)
            del copies[before:]
            return out
        trk.flower.compute_flow = unseen
        Hs, metas = trk.track(W._stub_frame(2))
        torch.cuda.synchronize()
    assert Hs.shape == (K, 3, 3) and not any(m.lost for m in metas) and metas[0].chain_window[2:] != (SH, SW)
    return proxy.calls, copies


def test_launches_and_reads_do_not_depend_on_k(monkeypatch):
    monkeypatch.setenv("WOFT_FUSED", "1")
    calls1, copies1 = _trace_one_track(1)
    calls8, copies8 = _trace_one_track(8)
    assert calls1 == calls8, (calls1, calls8)
    planar = [c for c in calls1 if c not in ("woft_flow_chain_fold_window", "woft_crop_u8")]
    assert planar == ["woft_chain_tc_multi_window", "woft_tc_select_multi", "woft_hfit_batched", "woft_inlier_frac_batched",
                      "woft_mask_bbox_multi"], planar
    assert calls1.count("woft_flow_chain_fold_window") == 3                      # (frame 2 of deltas (None, 1, 2, 4): 0, 1 and 0 again)
    assert copies1 == copies8 == ["copy_", "cpu"], (copies1, copies8)           # the planar block's read, the one box read


# ---- 8. the plans the provider keeps ----------------------------------------------------------------------------------------------------
def test_drifting_targets_leave_a_bounded_number_of_plans(monkeypatch):
    monkeypatch.setenv("WOFT_FUSED", "1")
    DH, DW, deltas = W.DH, W.DW, (None, 1, 2)
    conf = W._tracker_config("WOFT_chained_multi_window.py", "weighted", chain_deltas=deltas, chain_window_min=64, chain_window_quantum=32)
    conf.flow_config.iters = 2
    trk = conf.tracker_class(conf)
    big = synth.make_template(DH + 32, DW + 32, seq_id=6)
    frame = lambda t: np.ascontiguousarray(big[16:16 + DH, 16 + t:16 + t + DW])
    masks = [np.zeros((DH, DW), np.uint8) for _ in range(2)]
    masks[0][30:66, 20:60] = 255
    masks[1][50:80, 70:100] = 255
    trk.init(frame(0), masks)
    # the poses are scripted, whatever the seeded weights make of the frames: the targets drift and grow, so the union window's
    # quantised size changes every few frames
    step = {"t": 0}

    def scripted(H, good, state=None):
        t, k = step["t"], next(i for i, T in enumerate(trk._targets) if T is state)
        g = 1.0 + 0.06 * t
        to_frame = np.array([[g, 0, (8.0 + 3 * k) * t], [0, g, (4.0 + 2 * k) * t], [0, 0, 1.0]])
        state.prev_H2init = np.linalg.inv(to_frame)
    trk._set_pose = scripted
    sizes = {trk.chain_window[2:]}
    for t in range(1, 13):
        step["t"] = t
        trk.track(frame(t))
        sizes.add(trk.chain_window[2:])
        assert len(trk.flower.engine._plans) <= len(deltas) + 2, (t, sorted(trk.flower.engine._plans))
    torch.cuda.synchronize()
    print(f"{len(sizes)} window sizes over 12 frames, {len(trk.flower.engine._plans)} plans kept: {sorted(trk.flower.engine._plans)}")
    assert len(sizes) >= 4


# ---- 9. the fall-back -----------------------------------------------------------------------------------------------------------------
def test_with_no_contributing_target_the_previous_window_stays(monkeypatch):
    monkeypatch.setenv("WOFT_FUSED", "1")
    masks = [_rect_mask(MASK_A), _rect_mask(MASK_B)]
    trk = _two_motion_tracker(masks)
    for t in range(1, S_FRAMES + 1):
        trk.track(W._stub_frame(t))
    last, R0 = trk.chain_window, trk.multi.rect0
    assert last != R0
    calls = []
    real = ops.mask_bbox_multi

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "mask_bbox_multi", counted)

    def follow(*poses):
        trk.multi.track(W._stub_frame(1))                                        # (a frame whose window is still to be named)
        for T, P in zip(trk._targets, poses):
            T.prev_H2init = np.asarray(P, dtype=np.float64)
        del calls[:]
        trk._follow()
        return trk.chain_window, len(calls)
    singular = [[1.0, 2, 3], [2, 4, 6], [0, 0, 1]]
    nan = [[1.0, 0, 0], [0, 1, 0], [0, 0, np.nan]]
    far = [[1.0, 0, 5000], [0, 1, 0], [0, 0, 1]]                                 # the mask is carried out of the frame: nothing set
    eye = np.eye(3)
    chain = lambda *boxes: window.chain_rect(window.union_box(boxes), 0.25, SW, SH, 16, 32)
    box = lambda r, dx=0: window.Box(r[1] + dx, r[0], r[3], r[2])
    assert follow(singular, singular) == (last, 0)                               # no contributor, and no launch
    assert follow(nan, singular) == (last, 0)
    assert follow(far, far) == (last, 1)                                         # measured: nothing set
    assert follow(singular, far) == (last, 1)
    assert follow(eye, eye) == (R0, 0)                                           # the template boxes, no launch
    assert follow(eye, singular) == (chain(box(MASK_A)), 0)                      # one contributor alone
    shift = [[1.0, 0, -16], [0, 1, 0], [0, 0, 1]]                                # cur -> init by -16: the mask sits 16 px to the right
    assert follow(eye, shift) == (chain(box(MASK_A), box(MASK_B, 16)), 1)
    assert follow(far, shift) == (chain(box(MASK_B, 16)), 1)
