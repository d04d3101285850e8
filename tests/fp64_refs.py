"""Plain high-precision restatements of the per-frame kernels between the flow and the pose (a helper of the fp64 tests, not a
conftest): the homography fit, the inlier count, the weight head's mean channel and closing 1x1 conv, the bilinear x8 upsampling
with its crop, and the tracker's keep rule + Sobol selection on the crop geometry.  Everything here is float64 numpy / torch
(or exact integer logic); the GPU tests compare the HIP kernels against these, with tolerances derived from the kernels' own
fp32 rounding."""
import numpy as np
import torch

from oracle import hfit_ref, raft_ref

U32 = 2.0 ** -24                     # unit round-off of float32
U64 = 2.0 ** -53                     # unit round-off of float64


def _t64(x):
    if x is None:
        return None
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    return t.detach().cpu().to(torch.float64)


# ---- homography fit ----------------------------------------------------------------------------------------------------------
def fit(pa, pb, w=None):
    """Weighted inhomogeneous DLT (least_squares_H.py:142-210) in float64: pa, pb (N, 2), w (N,) or None -> (3, 3) float64.
    oracle.hfit_ref keeps the dtype of its inputs throughout; the one float32 constant in it is kornia's sqrt(2) of the
    Hartley scale, which the kernel uses too (sqrtf(2.0f))."""
    a, b = _t64(pa)[None], _t64(pb)[None]
    return hfit_ref.find_homography_nonhomogeneous_QR(a, b, None if w is None else _t64(w)[None])[0].numpy()


def fit_irls(pa, pb, w=None, huber_k=None, n_iter=5):
    """IRLS (least_squares_H.py:280-346) in float64 with the L1 loss (huber_k None) or Huber(k)."""
    a, b = _t64(pa)[None], _t64(pb)[None]
    fn = hfit_ref.IRLSq_L1 if huber_k is None else (lambda r: hfit_ref.IRLSq_Huber(r, k=huber_k))
    return hfit_ref.find_homography_IRLSq_QR(a, b, None if w is None else _t64(w)[None], reweighting_fn=fn,
                                             n_iter=n_iter)[0].numpy()


def box_corners(pa):
    """The 4 corners of the bounding box of the points pa (N, 2): where a fit's error is measured."""
    p = np.asarray(pa, np.float64)
    lo, hi = p.min(0), p.max(0)
    return np.array([[lo[0], lo[1]], [hi[0], lo[1]], [hi[0], hi[1]], [lo[0], hi[1]]])


def corner_err(Ha, Hb, corners):
    """max |H_a c - H_b c| over the corners (N, 2), in pixels, in float64."""
    c = np.concatenate([np.asarray(corners, np.float64), np.ones((len(corners), 1))], 1).T
    pa, pb = np.asarray(Ha, np.float64) @ c, np.asarray(Hb, np.float64) @ c
    return float(np.abs(pa[:2] / pa[2] - pb[:2] / pb[2]).max())


def residuals(pa, pb, w, sol, norm):
    """Rows of A x - b (least_squares_H.py:334) in float64 for a solution `sol` (8,) of the normalised system and the
    normalisation norm = (s1, t1x, t1y, s2, t2x, t2y): (2N,) interleaved x / y rows, and per row the magnitude
    sum_k |A_ik| |x_k| + |b_i| with every normalised coordinate replaced by |s a| + |t| -- the size of what an fp32
    evaluation rounds (s a + t cancels: its rounding error is relative to |s a| + |t|, not to the result)."""
    a, b = np.asarray(pa, np.float64), np.asarray(pb, np.float64)
    s1, t1x, t1y, s2, t2x, t2y = (float(v) for v in norm[:6])
    x = np.asarray(sol, np.float64)
    wr = None if w is None else np.repeat(np.asarray(w, np.float64), 2)

    def system(x1, y1, x2, y2):
        z, o = np.zeros_like(x1), np.ones_like(x1)
        ax = np.stack([z, z, z, -x1, -y1, -o, y2 * x1, y2 * y1], 1)
        ay = np.stack([x1, y1, o, z, z, z, -x2 * x1, -x2 * y1], 1)
        A, rhs = np.stack([ax, ay], 1).reshape(-1, 8), np.stack([-y2, x2], 1).reshape(-1)
        return (A, rhs) if wr is None else (A * wr[:, None], rhs * wr)
    A, rhs = system(s1 * a[:, 0] + t1x, s1 * a[:, 1] + t1y, s2 * b[:, 0] + t2x, s2 * b[:, 1] + t2y)
    Am, rm = system(abs(s1 * a[:, 0]) + abs(t1x), abs(s1 * a[:, 1]) + abs(t1y), abs(s2 * b[:, 0]) + abs(t2x),
                    abs(s2 * b[:, 1]) + abs(t2y))
    return A @ x - rhs, np.abs(Am) @ np.abs(x) + np.abs(rm)


# ---- inlier count --------------------------------------------------------------------------------------------------------------
def proj_dist(H, pa, pb, eps=1e-8):
    """|proj(H, a) - b| in float64 with kornia's from_homogeneous eps rule (scale = 1 / (z + eps) where |z| > eps, else 1),
    least_squares_H.py:474-489."""
    a, b = np.asarray(pa, np.float64), np.asarray(pb, np.float64)
    Hm = np.asarray(H, np.float64).reshape(3, 3)
    p = np.concatenate([a, np.ones((len(a), 1))], 1) @ Hm.T
    z = p[:, 2]
    sc = np.where(np.abs(z) > eps, 1.0 / (z + eps), 1.0)
    return np.sqrt(((sc[:, None] * p[:, :2] - b) ** 2).sum(1))


def proj_err_bound(H, pa, pb):
    """A bound on |d32 - d64| per point, d32 being the distance evaluated in float32 from float32 H and points: each of px,
    py, pz is a 3-term fp32 dot product (error <= 4u sum|terms|), the division by pz scales those errors by 1/|pz| and the
    subtraction and norm add a few u of the operands.  Large only where |pz| is small (near the horizon line)."""
    a, b = np.asarray(pa, np.float64), np.asarray(pb, np.float64)
    Hm = np.asarray(H, np.float64).reshape(3, 3)
    ah = np.concatenate([a, np.ones((len(a), 1))], 1)
    p, mag = ah @ Hm.T, np.abs(ah) @ np.abs(Hm).T
    z = np.abs(p[:, 2]) + 1e-300
    proj = np.abs(p[:, :2]) / z[:, None]
    e = (4 * U32 * mag[:, :2] + proj * 4 * U32 * mag[:, 2:3]) / z[:, None] + 2 * U32 * (proj + np.abs(b))
    return 2 * np.sqrt((e ** 2).sum(1)) + 4 * U32 * proj_dist(H, pa, pb)


def inlier_count(H, pa, pb, thr, band=1e-4):
    """(count, lo, hi): count = #(d <= thr) in float64; the kernel's float32 count must lie in [lo, hi], where the points
    within max(band * thr, proj_err_bound) of the threshold may fall either way."""
    d = proj_dist(H, pa, pb)
    tol = np.maximum(band * thr, proj_err_bound(H, pa, pb))
    return int((d <= thr).sum()), int((d <= thr - tol).sum()), int((d <= thr + tol).sum())


# ---- weight head glue -----------------------------------------------------------------------------------------------------------
def mean_channel(f1, f2):
    """The weight head's mean-response channel, mean_q <f1[p], f2[q]> / sqrt(C) (weighted_raft.py:358-361), in float64:
    f1 (P, C), f2 (Q, C) -> (P,)."""
    a, b = _t64(f1), _t64(f2)
    return ((a @ b.T).mean(1) / np.sqrt(a.shape[1])).numpy()


def wh_reduce(act, w, bias):
    """out[p] = bias + mean_t <w, act[p, t]> in float64: act (P, T, C), w (C,) -> (P,); and the magnitude
    sum_t |w| . |act[p, t]| / T that bounds an fp32 evaluation."""
    a, ww = _t64(act), _t64(w)
    return (float(bias) + (a @ ww).mean(1)).numpy(), ((a.abs() @ ww.abs()).mean(1)).numpy()


# ---- bilinear x8 upsampling -----------------------------------------------------------------------------------------------------
def upflow8_crop(flow, crop, h, w):
    """raft_ref.upflow8 (utils/utils.py:82-84: bilinear, align_corners=True, times 8) in float64, then the window
    (crop_top, crop_left, h, w): flow (1, C, hf, wf) -> (C, h, w)."""
    up = raft_ref.upflow8(_t64(flow))
    return up[0, :, crop[0]:crop[0] + h, crop[1]:crop[1] + w].numpy()


# ---- correspondence keep rule + Sobol selection ---------------------------------------------------------------------------------
def keep_rule(dst, tmask, pwmask, gh, gw, check_dst=True):
    """`_mask_coords` / `_mask_coords_flow` (YAOF_tracker_single_control.py:287-327) on the flow grid gh x gw, with masks
    of the frame's size mh x mw (gh <= mh, gw <= mw; padding_mode 'crop' makes the grid the frame cropped at the bottom
    right): source pixel i = y * gw + x reads tmask[y][x]; the target (dx, dy) is out when dx < 0, dy < 0, rint(dx) >= mw
    or rint(dy) >= mh, and NaN is out; else pwmask[rint(dy)][rint(dx)] decides.  dst (2, gh*gw) -> bool (gh*gw,)."""
    tmask = np.asarray(tmask)
    mh, mw = tmask.shape
    n = gh * gw
    i = np.arange(n)
    keep = tmask[i // gw, i % gw] != 0
    if check_dst:
        d = np.asarray(dst, np.float32).reshape(2, n)
        dx, dy = d[0], d[1]
        with np.errstate(invalid="ignore"):
            oob = ~(dx >= 0) | ~(dy >= 0) | (np.rint(dx) >= mw) | (np.rint(dy) >= mh)
        keep &= ~oob
        if pwmask is not None:
            pw = np.asarray(pwmask).reshape(mh, mw)
            ry = np.where(keep, np.rint(dy), 0).astype(np.int64)
            rx = np.where(keep, np.rint(dx), 0).astype(np.int64)
            keep &= pw[ry, rx] != 0
    return keep


def sobol_ranks(N, u):
    """The subsampler's picked ranks (configs/..._wLSq.py:31-53): the distinct rint(float32(N) * u_k) below N, increasing;
    every rank when there are no draws or at least N of them."""
    u = np.asarray(u, np.float32)
    if u.size == 0 or u.size >= N:
        return np.arange(N)
    r = np.rint(np.float32(N) * u).astype(np.int64)
    return np.unique(r[(r >= 0) & (r < N)])


def select(dst, w, tmask, pwmask, gh, gw, u, cap):
    """tc_select's outputs: (pa, pb, w_out, count[0], count[1]) for the first min(M, cap) selected correspondences."""
    keep = keep_rule(dst, tmask, pwmask, gh, gw)
    kept = np.nonzero(keep)[0]
    chosen = kept[sobol_ranks(len(kept), u)][:cap]
    d = np.asarray(dst, np.float32).reshape(2, -1)
    pa = d[:, chosen].T
    pb = np.stack([chosen % gw, chosen // gw], 1).astype(np.float32)
    wo = np.ones(len(chosen), np.float32) if w is None else np.asarray(w, np.float32).reshape(-1)[chosen]
    return pa, pb, wo, len(chosen), len(kept)
