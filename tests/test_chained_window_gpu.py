"""The chained trackers on search windows, on the GPU: WindowedMultiFlowTracker on the real provider against
the pieces applied by hand (crop or window warp, compute_flow, chain_fold_window), byte for byte; WOFTChainedWindow with whole-frame
windows against WOFTChained, byte for byte, on both solver back ends; WOFTChainedWindow on a stub provider with a known motion that
carries the target out of its first window; the number of plans the provider keeps under a drifting box."""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from woft_amd import ops, synth, window  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
ITERS, MASK_HEAD = 3, [(64, 3)]


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ibits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _patch_flow_config(fc, raft_type, padding_mode=None):
    """Seeded synthetic weights, few iterations; the config's other keys stay."""
    masked = raft_type == "weighted_masked"
    fc.model = synth.make_state_dict(seed=7, weighted=raft_type != "orig", mask_head_structure=MASK_HEAD if masked else None)
    fc.raft_type, fc.iters, fc.precision = raft_type, ITERS, "bf16x3"
    if masked:
        fc.class_params.mask_estimation, fc.class_params.mask_head_structure = True, MASK_HEAD
    if padding_mode:
        fc.padding_mode = padding_mode
    return fc


def _flow_config(raft_type, padding_mode=None):
    from pytracking.utils.config import load_config
    return _patch_flow_config(load_config(ROOT / "pytracking" / "optical_flow" / "configs" / "v2_SNOB_large_g05_RAFT.py"), raft_type,
                              padding_mode)


# ---- 1. the dense tracker on the real provider ----------------------------------------------------------------------------------
DH, DW, D_DELTAS = 192, 256, (None, 1, 2)


def _drift_rect(t):
    """The window of frame t: a 60 x 50 box drifting by (9, 5) px a frame, chain_window_min 64, quantum 32."""
    return window.chain_rect(window.Box(70 + 9 * t, 50 + 5 * t, 60, 50), 0.25, DW, DH, 32, 64)


@pytest.fixture(scope="module")
def dense_frames():
    big = synth.make_template(DH + 32, DW + 32, seq_id=5)
    return [np.ascontiguousarray(big[16 - t:16 - t + DH, 16 + 2 * t:16 + 2 * t + DW]) for t in range(5)]


@pytest.mark.parametrize("raft_type,prewarp_at,deltas", [("weighted", 3, D_DELTAS), ("weighted_masked", None, D_DELTAS),
                                                         ("weighted", None, (2, 1))])
def test_dense_tracker_equals_the_pieces_applied_by_hand(dense_frames, raft_type, prewarp_at, deltas):
    """(None, 1, 2) is the issue's case; on seeded random weights its direct candidate is the cheapest everywhere, so (2, 1) -- from
    frame 3 on two real chains on different rectangles compete -- is run as well."""
    from woft_amd import WindowedMultiFlowTracker, chain_fold_window
    fc = _flow_config(raft_type)
    prov = fc.of_class(fc)
    trk = WindowedMultiFlowTracker(prov, deltas=deltas)
    rects = {t: _drift_rect(t) for t in range(5)}
    R0 = rects[0]
    assert len(set(rects.values())) >= 3 and all(r[2] % 32 == 0 and r[3] % 32 == 0 for r in rects.values()), rects
    frames = [cuda(f) for f in dense_frames]
    trk.init(frames[0], R0)
    th, tw = R0[2:]
    z = lambda *s: torch.zeros(*s, device="cuda")
    stored = {0: (z(2, th, tw), z(1, th, tw), torch.ones(1, th, tw, device="cuda"))}
    Hpre = np.array([[1.0, 0.004, -2.0], [-0.003, 1.0, 1.0], [1e-5, 0.0, 1.0]])
    wins = set()
    for t in range(1, 5):
        pre = Hpre if t == prewarp_at else None
        out = trk.track(frames[t], prewarp_H=pre)
        trk.set_rect(rects[t])
        keep = {n: getattr(out, n).clone() for n in ("flow", "cost", "vis", "occluded", "sel")}
        assert out.rect == R0 and out.frame_index == t and tuple(out.flow.shape) == (2, th, tw)
        best = None
        for k, d in enumerate(deltas):
            s = 0 if d is None else t - d
            if s < 0:
                continue
            B = R0 if d is None else rects[s]
            src, post = ops.crop_u8(frames[s], B), None
            if d is None and pre is not None:
                dst = torch.empty_like(src)
                ops.warp_perspective_window_u8(frames[t], pre, B, dst, None)
                post = np.linalg.inv(pre)
                post = post / post[2, 2]
            else:
                dst = ops.crop_u8(frames[t], B)
            res = prov.compute_flow(src, dst, mode="flow")
            assert len(res) == (3 if raft_type == "weighted_masked" else 2)
            best = chain_fold_window(best, None if d is None else stored[s], tuple(res), k, R0, B, post_H=post)
        stored[t] = best[:3]
        hand = dict(flow=best[0], cost=best[1], vis=best[2], occluded=best[2] < 0.5, sel=best[3])
        for n in hand:
            assert torch.equal(_ibits(getattr(out, n)), _ibits(hand[n])), (raft_type, t, n)
            assert torch.equal(_ibits(getattr(out, n)), _ibits(keep[n])), "a further compute_flow changed the tracker's result"
        sel = set(torch.unique(out.sel).tolist())
        wins |= sel
        print(f"{raft_type} {deltas} frame {t}: candidates that won somewhere {sorted(sel)}, {int((out.sel < 0).sum())} of {th * tw} pixels "
              "without a valid chain")
        assert sel - {-1}
        # the ring: frames t-1 and t by their rects, results on R0; its tensors are the tracker's own
        assert sorted(trk._ring) == list(range(max(0, t - 1), t + 1))
        own = {x.data_ptr() for o in prov._out.values() for x in o.values() if isinstance(x, torch.Tensor)}
        for s, (crop, rect, r) in trk._ring.items():
            assert rect == rects[s] and tuple(crop.shape) == rect[2:] + (3,) and tuple(r[0].shape) == (2, th, tw)
            assert not own & {x.data_ptr() for x in (crop,) + tuple(r)}
            assert crop.data_ptr() not in {f.data_ptr() for f in frames}
    if deltas == (2, 1):
        assert {0, 1} <= wins, wins


# ---- 2. whole-frame windows: WOFTChained, byte for byte -------------------------------------------------------------------------
def _tracker_config(name, raft_type, **keys):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / name)
    _patch_flow_config(conf.flow_config, raft_type, "RAFT")
    for k, v in keys.items():
        setattr(conf, k, v)
    return conf


@pytest.mark.parametrize("fused", [True, False])
def test_whole_frame_windows_return_woftchaineds_bytes(monkeypatch, fused):
    monkeypatch.setenv("WOFT_FUSED", "1" if fused else "0")
    Hh, Ww = 128, 160
    template = synth.make_template(Hh, Ww, seq_id=3)
    frames = [synth.make_frame(template, t) for t in (1, 2, 3, 4)]
    mask = synth.make_init_mask(Hh, Ww)
    results = []
    for name, keys in (("WOFT_chained.py", {}), ("WOFT_chained_window.py", dict(search_window_margin=None, chain_prewarp=False))):
        conf = _tracker_config(name, "weighted", chain_deltas=(None, 1, 2), **keys)
        trk = conf.tracker_class(conf)
        assert (trk._fused is not None) == fused
        trk.init(template, mask)
        results.append([trk.track(f) for f in frames])
        if keys:
            assert trk.chain_window == (0, 0, Hh, Ww) and trk.multi.rect0 == (0, 0, Hh, Ww)
    for t, ((Ha, ma), (Hb, mb)) in enumerate(zip(*results), 1):
        assert np.array_equal(Ha, Hb), t
        assert mb.chain_window == (0, 0, Hh, Ww)
        for n, v in vars(ma).items():
            w = getattr(mb, n)
            if n == "solver_decision":
                assert w.startswith(v) and "search windows" in w
            elif isinstance(v, np.ndarray):
                assert np.array_equal(v, w) and v.dtype == w.dtype, (t, n)
            else:
                assert v == w and type(v) is type(w), (t, n)
        assert set(vars(mb)) - set(vars(ma)) == {"chain_window"}
    assert any(not np.array_equal(Hm, np.eye(3)) and np.isfinite(Hm).all() for Hm, _ in results[0])


# ---- 3. known motion on a stub provider -----------------------------------------------------------------------------------------
SH, SW, S_FRAMES, S_DELTAS = 96, 128, 6, (None, 1, 2, 4)
BOUND_PX = 1e-2        # tests/test_chained_gpu.py's bound and derivation: fp32 rounding of coordinates below 128 is ~8e-6 per operation,
                       # six chain steps of about ten operations each stay under 1e-3 px; one order of margin.
MASK = (30, 20, 24, 32)                                                        # (y0, x0, rows, cols) of the template mask


def _motion(t):
    """A_t: frame 0 -> frame t: a small rotation and anisotropic scale about the mask's centre, and a translation of (6, 1.5) px
    a frame -- 36 px over the six frames, beyond the window's margin of 8 px."""
    c, s = np.cos(0.01 * t), np.sin(0.01 * t)
    L = np.array([[c, -s], [s, c]]) @ np.diag([1 + 0.004 * t, 1 - 0.003 * t])
    centre = np.array([35.5, 41.5])
    A = np.eye(3)
    A[:2, :2], A[:2, 2] = L, centre - L @ centre + np.array([6.0 * t, 1.5 * t])
    return A


def _stub_frame(t):
    ys, xs = np.mgrid[:SH, :SW]
    return np.stack([np.full((SH, SW), t), xs, ys], axis=-1).astype(np.uint8)


class _MotionProvider:
    """Analytic flows on crops.  Frames carry (frame index, x, y) in their channels, so a crop tells its frame and its origin.  The
    first call of every frame is the direct candidate (deltas[0] is None).  bad = 'direct': the direct flow is 5 px off with
    reliability logit -4, the chained flows are exact with +4; bad = 'chained': the other way round.  A pre-warped direct target
    (its pixels are the warp's: the origin is read from the source crop) gets the exact flow into the pre-warped frame,
    H_pre A_t p - p, with H_pre read from the tracker."""
    precision, precision_source = "stub", "stub"

    def __init__(self, cfg, bad):
        self.C, self.bad, self.pinned, self.calls, self._last_t, self.tracker, self.bound = cfg, bad, None, [], None, None, None

    def pin_source(self, img):
        self.pinned = img

    def bound_plans(self, n):
        self.bound = n

    def compute_flow(self, src, dst, mode=None, do_sigmoid=None, borrow=None, **kw):
        assert mode == "flow" and do_sigmoid is False and borrow is True and not kw and src.shape == dst.shape
        s, t = int(src[0, 0, 0]), int(dst[..., 0].max())
        x0, y0 = int(src[0, 0, 1]), int(src[0, 0, 2])
        rows, cols = src.shape[:2]
        direct, self._last_t = t != self._last_t, t
        Hpre = self.tracker.last_good_H2init if (direct and self.tracker.chain_prewarp) else np.eye(3)
        warped = not np.array_equal(Hpre, np.eye(3))
        if not warped:
            assert (int(dst[0, 0, 1]), int(dst[0, 0, 2])) == (x0, y0)         # (the same rect of both frames)
        self.calls.append((s, t, (y0, x0, rows, cols), direct, warped))
        ys, xs = np.mgrid[y0:y0 + rows, x0:x0 + cols].astype(np.float64)
        M = Hpre @ _motion(t) @ np.linalg.inv(_motion(s))
        den = M[2, 0] * xs + M[2, 1] * ys + M[2, 2]
        flow = np.stack([(M[0, 0] * xs + M[0, 1] * ys + M[0, 2]) / den - xs, (M[1, 0] * xs + M[1, 1] * ys + M[1, 2]) / den - ys])
        off = direct == (self.bad == "direct")
        if off:
            flow += np.array([3.0, 4.0])[:, None, None]
        return cuda(flow.astype(np.float32)), torch.full((1, rows, cols), -4.0 if off else 4.0, device="cuda")


def _stub_mask():
    m = np.zeros((SH, SW), np.uint8)
    m[MASK[0]:MASK[0] + MASK[2], MASK[1]:MASK[1] + MASK[3]] = 255
    return m


def _corner_error(Hm, t):
    y0, x0, rows, cols = MASK
    c = np.array([[x0, y0, 1], [x0 + cols - 1, y0, 1], [x0 + cols - 1, y0 + rows - 1, 1], [x0, y0 + rows - 1, 1.0]]).T
    a, b = Hm @ c, np.linalg.inv(_motion(t)) @ c
    return float(np.abs(a[:2] / a[2] - b[:2] / b[2]).max())


def _stub_run(bad, prewarp):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained_window.py")
    conf.flow_config.of_class = lambda fc: _MotionProvider(fc, bad)
    conf.chain_deltas, conf.chain_window_min, conf.chain_window_quantum, conf.chain_prewarp = S_DELTAS, 32, 16, prewarp
    trk = conf.tracker_class(conf)
    trk.flower.tracker = trk
    trk.init(_stub_frame(0), _stub_mask())
    return trk, [trk.track(_stub_frame(t)) for t in range(1, S_FRAMES + 1)]


def test_known_motion_the_window_follows_the_target():
    trk, res = _stub_run("direct", prewarp=False)
    R0 = trk.multi.rect0
    box = window.Box(MASK[1], MASK[0], MASK[3], MASK[2])
    assert R0 == window.chain_rect(box, 0.25, SW, SH, 16, 32) and R0[2] % 16 == 0 and R0[3] % 16 == 0 and R0[:2] != (0, 0)
    assert trk.flower.bound == len(S_DELTAS) + 1
    n_mask = MASK[2] * MASK[3]
    rects, errs = {0: R0}, []
    for t, (Hm, meta) in enumerate(res, 1):
        assert not meta.lost and meta.global_H_success and np.array_equal(Hm, meta.H_global_cur2init)
        assert meta.chain_hist.sum() + meta.chain_invalid + meta.chain_occluded == n_mask
        rects[t] = meta.chain_window
        errs.append(_corner_error(Hm, t))
        print(f"frame {t}: window {meta.chain_window}, kept {meta.n_kept}, chain_hist {meta.chain_hist.tolist()}, "
              f"corner error {errs[-1]:.2e} px")
        if t >= 2:                                                             # (frame 1 has the direct candidate's 5 px alone ... and the chain from frame 0)
            assert errs[-1] <= BOUND_PX, (t, errs[-1])
            assert meta.chain_hist[0] == 0 and meta.n_kept == n_mask
        # the window is the rule applied to the mask carried by the pose that was returned
        assert all(0 <= v for v in rects[t]) and rects[t][0] + rects[t][2] <= SH and rects[t][1] + rects[t][3] <= SW
    assert errs[0] <= BOUND_PX                                                 # (frame 1: the exact chain through frame 0 beats the direct flow)
    assert rects[S_FRAMES] != R0 and rects[S_FRAMES][1] >= R0[1] + 24         # (36 px of motion: the window has moved with the target)
    # the provider was asked for the schedule's crops at the expected rects, the direct one first
    want = [(s, t, R0 if not chained else rects[s], not chained, False)
            for t in range(1, S_FRAMES + 1) for _, s, chained in trk.multi.schedule(t)]
    assert trk.flower.calls == want
    print(f"known motion, frames 1..{S_FRAMES}: largest corner error {max(errs):.2e} px (bound {BOUND_PX} px)")


def test_known_motion_the_prewarped_direct_flow_recovers_the_pose_when_every_chain_is_unreliable():
    trk, res = _stub_run("chained", prewarp=True)
    n_mask = MASK[2] * MASK[3]
    errs = []
    for t, (Hm, meta) in enumerate(res, 1):
        errs.append(_corner_error(Hm, t))
        print(f"frame {t}: window {meta.chain_window}, kept {meta.n_kept}, chain_hist {meta.chain_hist.tolist()}, "
              f"corner error {errs[-1]:.2e} px")
        assert not meta.lost and errs[-1] <= BOUND_PX, (t, errs[-1])
        assert meta.chain_hist[0] == meta.n_kept == n_mask                     # (the direct candidate wins under the whole mask)
    direct = [c for c in trk.flower.calls if c[3]]
    assert [c[4] for c in direct] == [False] + [True] * (S_FRAMES - 1)        # (pre-warped from the first non-identity pose on)
    assert all(c[2] == trk.multi.rect0 for c in direct)


# ---- 4. the plans the provider keeps --------------------------------------------------------------------------------------------
def test_a_drifting_box_leaves_a_bounded_number_of_plans():
    from woft_amd import WindowedMultiFlowTracker
    fc = _flow_config("weighted", "RAFT")
    fc.iters = 2
    prov = fc.of_class(fc)
    deltas = (None, 1, 2)
    trk = WindowedMultiFlowTracker(prov, deltas=deltas)
    big = synth.make_template(DH + 32, DW + 32, seq_id=6)
    frame = lambda t: np.ascontiguousarray(big[16:16 + DH, 16 + t:16 + t + DW])
    # a box that drifts and grows: the quantised sizes change every few frames
    rect = lambda t: window.chain_rect(window.Box(20 + 8 * t, 30 + 4 * t, 40 + 9 * t, 36 + 6 * t), 0.25, DW, DH, 32, 64)
    trk.init(frame(0), rect(0))
    sizes = {rect(0)[2:]}
    for t in range(1, 13):
        trk.track(frame(t))
        trk.set_rect(rect(t))
        sizes.add(rect(t)[2:])
        assert len(prov.engine._plans) <= len(deltas) + 2, (t, sorted(prov.engine._plans))
    torch.cuda.synchronize()
    print(f"{len(sizes)} window sizes over 12 frames, {len(prov.engine._plans)} plans kept: {sorted(prov.engine._plans)}")
    assert len(sizes) >= 4


def test_a_singular_pose_or_an_empty_carried_mask_keeps_the_previous_window():
    trk, _ = _stub_run("direct", prewarp=False)
    last = trk.chain_window
    assert last != trk.multi.rect0

    def follow(pose):
        trk.multi.track(_stub_frame(1))                                        # (a frame whose window is still to be named)
        trk.prev_H2init = pose
        trk._follow()
        return trk.chain_window
    assert follow(np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]])) == last       # singular: no inverse
    assert follow(np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, np.nan]])) == last
    assert follow(np.array([[1.0, 0, 5000], [0, 1, 0], [0, 0, 1]])) == last    # the mask is carried out of the frame: nothing set
    assert follow(np.eye(3)) == trk.multi.rect0                                # the identity: the template's own box, no launch
    shifted = follow(np.array([[1.0, 0, -16], [0, 1, 0], [0, 0, 1]]))          # cur -> init by -16: the mask sits 16 px to the right
    assert shifted == (trk.multi.rect0[0], trk.multi.rect0[1] + 16) + trk.multi.rect0[2:]
