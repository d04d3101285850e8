"""Helpers of the multi-target chained tracker's tests (test infrastructure): fold results with planted
values, mask sets, a stub flow provider with analytic affine motions, byte comparisons of tracker results and a counter of the
library's entry-point calls.  Nothing here computes an expected value: every test compares the multi-target path with the
existing single-target entry points."""
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- kernel inputs ----------------------------------------------------------------------------------------------------------------
def make_fold(h, w, n_cand=5, seed=0, vis_thr=0.5, plant=True):
    """A fold result (flow (2, h, w), cost, vis (h, w) fp32, sel (h, w) int32) with, when plant, one pixel each of: sel -1, sel 128,
    NaN flow x, NaN flow y, infinite cost, NaN vis, vis exactly at vis_thr, vis just below it, sel 127; and a flow that sends a
    band of pixels out of the frame on every side."""
    rng = np.random.default_rng(seed)
    flow = rng.normal(0.0, 3.0, (2, h, w)).astype(np.float32)
    flow[0, :, :2] -= 9.0                                   # (out of frame on the left ...)
    flow[0, :, -2:] += 9.0
    flow[1, :2] -= 9.0
    flow[1, -2:] += 9.0
    cost = rng.uniform(0.0, 3.0, (h, w)).astype(np.float32)
    vis = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    sel = rng.integers(0, n_cand, (h, w)).astype(np.int32)
    if plant:
        at = rng.choice(h * w, 9, replace=False)
        f = lambda a: a.reshape(-1)
        f(sel)[at[0]], f(sel)[at[1]], f(sel)[at[8]] = -1, 128, 127
        f(flow[0])[at[2]], f(flow[1])[at[3]] = NAN, NAN
        f(cost)[at[4]], f(vis)[at[5]] = INF, NAN
        f(vis)[at[6]] = np.float32(vis_thr)
        f(vis)[at[7]] = np.nextafter(np.float32(vis_thr), np.float32(0))
    return dict(flow=flow, cost=cost, vis=vis, sel=sel)


def make_masks(mh, mw, K, seed=0):
    """K uint8 masks (0 / 255) of mh x mw: rectangles that overlap; with K >= 3, mask 1 is empty and mask 2 covers everything."""
    rng = np.random.default_rng(1000 + seed)
    masks = []
    for t in range(K):
        m = np.zeros((mh, mw), np.uint8)
        y0, x0 = int(rng.integers(0, mh // 2)), int(rng.integers(0, mw // 2))
        m[y0:y0 + int(rng.integers(2, mh // 2 + 1)), x0:x0 + int(rng.integers(2, mw // 2 + 1))] = 255
        masks.append(m)
    masks[0][mh // 4:3 * mh // 4, mw // 4:3 * mw // 4] = 255          # (the middle: overlaps most of the others)
    if K >= 3:
        masks[1][:] = 0
        masks[2][:] = 255
    return masks


def survivor_masks(mh, mw):
    """Four masks for the selection: none of its pixels survives (empty), 3 pixels, 48 pixels, most of the frame; the last two
    overlap.  All stay 4 pixels off the frame's border, where make_fold's flow leaves the frame."""
    m = [np.zeros((mh, mw), np.uint8) for _ in range(4)]
    m[1][6, 6:9] = 1
    m[2][8:14, 10:18] = 1
    m[3][4:mh - 4, 4:mw - 4] = 1
    return m


# ---- the stub provider --------------------------------------------------------------------------------------------------------------
SH, SW, S_FRAMES, S_DELTAS = 48, 64, 6, (None, 1, 2, 4)


def motion(t):
    """Frame 0 -> frame t: a 3 x 3 float64 affine map, a slow rotation and anisotropic scale about the frame's centre plus a drift
    along y (under 0.25 px of x-displacement along the column x = 32)."""
    c, s = np.cos(0.012 * t), np.sin(0.012 * t)
    L = np.array([[c, -s], [s, c]]) @ np.diag([1 + 0.003 * t, 1 - 0.004 * t])
    centre = np.array([32.0, 24.0])
    A = np.eye(3)
    A[:2, :2], A[:2, 2] = L, centre - L @ centre + np.array([0.0, 0.7 * t])
    return A


class AffineProvider:
    """A flow provider for MultiFlowTracker: a frame's pixel value is its index, the flow s -> t is motion(t) motion(s)^-1 p - p.
    The first flow asked for into a new frame is the direct candidate (deltas[0] is None): it carries reliability logit -4 and an
    offset of (3, 4) px, every other flow is exact with logit +4.  occlude 'left@3': visibility logit -6 on the left half of every
    flow into frame 3, +6 elsewhere."""
    precision, precision_source = "stub", "stub"

    def __init__(self, cfg, occlude=None):
        self.C, self.occlude, self.pinned, self.n_calls, self._last_t = cfg, occlude, None, 0, None

    def pin_source(self, img):
        self.pinned = img

    def compute_flow(self, src, dst, mode=None, do_sigmoid=None, borrow=None, **kw):
        import torch
        assert mode == "flow" and do_sigmoid is False and borrow is True and not kw
        s, t = int(src[0, 0, 0]), int(dst[0, 0, 0])
        direct, self._last_t = t != self._last_t, t
        self.n_calls += 1
        ys, xs = np.mgrid[:SH, :SW].astype(np.float64)
        M = motion(t) @ np.linalg.inv(motion(s))
        flow = np.stack([M[0, 0] * xs + M[0, 1] * ys + M[0, 2] - xs, M[1, 0] * xs + M[1, 1] * ys + M[1, 2] - ys])
        if direct:
            flow += np.array([3.0, 4.0])[:, None, None]
        out = [torch.from_numpy(flow.astype(np.float32)).cuda(), None]
        if self.C.raft_type != "orig":
            out[1] = torch.full((1, SH, SW), -4.0 if direct else 4.0, device="cuda")
        if self.C.raft_type == "weighted_masked":
            ml = torch.full((1, SH, SW), 6.0, device="cuda")
            if self.occlude == "left@3" and t == 3:
                ml[:, :, :SW // 2] = -6.0
            out.append(ml)
        return tuple(out)


def stub_masks():
    """One ordinary mask, one overlapping it, one of 1 x 3 pixels (never 4 correspondences: lost on every frame)."""
    a, b, c = (np.zeros((SH, SW), np.uint8) for _ in range(3))
    a[12:36, 16:48] = 255
    b[6:30, 8:36] = 255
    c[20, 30:33] = 255
    return [a, b, c]


def stub_frames():
    return np.zeros((SH, SW, 3), np.uint8), [np.full((SH, SW, 3), t, np.uint8) for t in range(1, S_FRAMES + 1)]


def stub_config(multi, raft_type="weighted", occlude=None, estimator=None):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / ("WOFT_chained_multi.py" if multi else "WOFT_chained.py"))
    conf.flow_config.raft_type = raft_type
    conf.flow_config.of_class = lambda fc: AffineProvider(fc, occlude)
    conf.chain_deltas = S_DELTAS
    if estimator is not None:
        conf.H_estimator = estimator
    return conf


# ---- comparisons --------------------------------------------------------------------------------------------------------------------
def same_value(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
                and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))
    return type(a) is type(b) and a == b


def assert_same_result(multi_res, single_res, tag=""):
    """multi_res: [(Hs (K, 3, 3), metas)] per frame; single_res: per target, [(H, meta)] per frame."""
    K = len(single_res)
    for f, (Hs, metas) in enumerate(multi_res, 1):
        assert isinstance(Hs, np.ndarray) and Hs.shape == (K, 3, 3) and Hs.dtype == np.float64 and len(metas) == K
        for t in range(K):
            H1, m1 = single_res[t][f - 1]
            assert np.array_equal(Hs[t], H1), (tag, "H", f, t, Hs[t], H1)
            a, b = vars(metas[t]), vars(m1)
            assert sorted(a) == sorted(b), (tag, f, t, sorted(a), sorted(b))
            for k in a:
                assert same_value(a[k], b[k]), (tag, k, f, t, a[k], b[k])


# ---- counting what a track() launches and reads --------------------------------------------------------------------------------------
class CountingLib:
    """Stands in for the loaded library (woft_amd._lib._lib): counts the calls of every entry point."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("woft_") or name.endswith("_ws_bytes"):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted
