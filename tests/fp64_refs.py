"""Plain high-precision restatements of the per-frame kernels between the flow and the pose (a helper of the fp64 tests, not a
conftest): the homography fit, the inlier count, the weight head's mean channel and closing 1x1 conv, the bilinear x8 upsampling
with its crop, the perspective warp / downscale of the frame, the tracker's keep rule + Sobol selection on the crop geometry,
and -- at the end -- the correlation lookup, the flow-head gather and the convex upsampling of the refinement loop.
Everything here is float64 numpy / torch
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


# ---- perspective warp, downscale: the per-frame image geometry -----------------------------------------------------------------
# The band of the classification rule: how far the kernel's fp32 value of one byte can lie from the fp64 value, derived (not
# measured) from csrc/warp_pixel.h; resize_linear_kernel interpolates the same way.  In units of 2^-24:
#   * the source coordinates are fp64 and the fractions fx, fy are rounded to fp32 once each: at most 2^-25 each, times a gradient
#     |t01 - t00| <= 255                                                                                    -> 2 * 127.5
#   * 1 - fx and 1 - fy are rounded (at most 2^-25, the values being <= 1) and then multiply a value <= 255   -> 2 * 127.5
#     (top and bot both carry the error of 1 - fx, but enter v with weights (1 - fy) + fy = 1: it counts once)
#   * top = t00 (1 - fx) + t01 fx is two products and a sum, each rounded to a value <= 255, so by at most half an ulp of a
#     number below 256, 2^-17 = 128 * 2^-24; bot likewise, and again the pair counts once                     -> 3 * 128
#   * v = top (1 - fy) + bot fy: two products and a sum                                                       -> 3 * 128
# Sum 1278 < 8 * 255 = 2040 (contraction to FMA only removes roundings).  The fp64 coordinates of the kernel and of numpy differ
# by some 1e-13 at most, times 255: nothing on this scale.
WARP_BAND = 8 * 255 * 2.0 ** -24
WARP_FAR = 1e9                       # a source coordinate beyond this (or not finite) is "nowhere": value 0, invalid


def warp_source64(h, w, Hm):
    """Source coordinates (sx, sy) and the denominator d of every destination pixel of an h x w frame, float64, with
    Hinv = np.linalg.inv(Hm) as ops takes it.  Where d == 0 both coordinates are +inf (never NaN, and nothing is divided by 0)."""
    Hi = np.linalg.inv(np.asarray(Hm, np.float64))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    d = Hi[2, 0] * xs + Hi[2, 1] * ys + Hi[2, 2]
    nx = Hi[0, 0] * xs + Hi[0, 1] * ys + Hi[0, 2]
    ny = Hi[1, 0] * xs + Hi[1, 1] * ys + Hi[1, 2]
    zero = d == 0
    safe = np.where(zero, 1.0, d)
    with np.errstate(over="ignore", under="ignore"):     # a tiny d may overflow to inf: that is a pixel "nowhere", as wanted
        sx, sy = nx / safe, ny / safe
    sx[zero], sy[zero] = np.inf, np.inf
    return sx, sy, d


def _warp_live(sx, sy):
    """Pixels whose source lies somewhere: finite and within WARP_FAR (comparisons only; inf compares without a warning)."""
    return (np.abs(sx) <= WARP_FAR) & (np.abs(sy) <= WARP_FAR)


def warp_linear64(img, Hm):
    """dst(x, y) = bilinear src(Hinv (x, y)) with a zero border, all in float64 and UNROUNDED: (v, sx, sy), v shaped like img.
    A pixel whose source is not finite or beyond WARP_FAR has value 0 (no inf or NaN is ever cast to an integer)."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    sx, sy, _ = warp_source64(h, w, Hm)
    live = _warp_live(sx, sy)
    sxl, syl = np.where(live, sx, -2.0), np.where(live, sy, -2.0)          # -2: every tap outside, value 0
    fx0, fy0 = np.floor(sxl), np.floor(syl)
    fx, fy = (sxl - fx0)[..., None], (syl - fy0)[..., None]
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    src = img.astype(np.float64).reshape(h, w, -1)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * ok[..., None]

    top = tap(y0, x0) * (1 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (1 - fx) + tap(y0 + 1, x0 + 1) * fx
    v = top * (1 - fy) + bot * fy
    v[~live] = 0.0
    return v.reshape(img.shape), sx, sy


def warp_valid64(sx, sy, h, w):
    """warp(ones) > 0: some tap inside the frame has positive weight, which is exactly -1 < sx < w and -1 < sy < h."""
    return _warp_live(sx, sy) & (sx > -1) & (sx < w) & (sy > -1) & (sy < h)


def warp_valid_excused(sx, sy, h, w, eps=1e-6):
    """Pixels whose validity fp32 may decide either way: sx within eps of -1 or w, sy within eps of -1 or h (there
    (float)(sx - floor(sx)) may round to 0 or 1)."""
    live = _warp_live(sx, sy)
    ex, ey = np.where(live, sx, 0.5), np.where(live, sy, 0.5)
    return (np.abs(ex + 1) < eps) | (np.abs(ex - w) < eps) | (np.abs(ey + 1) < eps) | (np.abs(ey - h) < eps)


def warp_nearest64(img, Hm):
    """src(rint(sx), rint(sy)), rounding half to even, 0 outside: (bytes shaped like img, sx, sy, inside) with inside (h, w) the
    pixels that read a source pixel."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    sx, sy, _ = warp_source64(h, w, Hm)
    live = _warp_live(sx, sy)
    rx = np.rint(np.where(live, sx, -2.0)).astype(np.int64)
    ry = np.rint(np.where(live, sy, -2.0)).astype(np.int64)
    inside = (rx >= 0) & (rx < w) & (ry >= 0) & (ry < h)
    src = img.reshape(h, w, -1)
    out = src[np.clip(ry, 0, h - 1), np.clip(rx, 0, w - 1)] * inside[..., None].astype(img.dtype)
    return out.reshape(img.shape), sx, sy, inside


def warp_nearest_excused(sx, sy, h, w, eps=1e-9):
    """Pixels whose nearest source pixel may legitimately differ: sx or sy within eps of a half-integer, where contraction to FMA
    in the fp64 coordinate can flip the tie -- and the source within a pixel of the frame (-1 < sx < w, -1 < sy < h): farther
    out both neighbours of the tie lie outside and the byte is 0 either way."""
    live = _warp_live(sx, sy)
    ex, ey = np.where(live, sx, 0.0), np.where(live, sy, 0.0)
    tie = (np.abs(ex - np.floor(ex) - 0.5) < eps) | (np.abs(ey - np.floor(ey) - 0.5) < eps)
    return tie & live & (sx > -1) & (sx < w) & (sy > -1) & (sy < h)


def resize_out_shape(h, w, factor):
    """(ho, wo) = int(round(. / factor)), Python's round: half to even."""
    return int(round(h / factor)), int(round(w / factor))


def resize_linear64(img, factor):
    """oracle.tracker_ref.resize_linear_u8's geometry (src = (dst + 0.5) * factor - 0.5, edge clamped, ho = int(round(h /
    factor))) with float64 interpolation, UNROUNDED, shaped (ho, wo[, c])."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    ho, wo = resize_out_shape(h, w, factor)

    def axis(n_out, n_in):
        f = (np.arange(n_out, dtype=np.float64) + 0.5) * float(factor) - 0.5
        i0 = np.floor(f)
        wt = f - i0
        i0 = i0.astype(np.int64)
        wt[i0 < 0] = 0.0
        i0 = np.clip(i0, 0, n_in - 1)
        wt[i0 >= n_in - 1] = 0.0
        return i0, np.minimum(i0 + 1, n_in - 1), wt

    y0, y1, wy = axis(ho, h)
    x0, x1, wx = axis(wo, w)
    src = img.astype(np.float64).reshape(h, w, -1)
    wxx, wyy = wx[None, :, None], wy[:, None, None]
    top = src[y0][:, x0] * (1 - wxx) + src[y0][:, x1] * wxx
    bot = src[y1][:, x0] * (1 - wxx) + src[y1][:, x1] * wxx
    return (top * (1 - wyy) + bot * wyy).reshape((ho, wo) + img.shape[2:])


def classify_bytes(v, g, band=WARP_BAND):
    """The classification rule for bilinear bytes: with v the fp64 value the byte g must satisfy floor(v + 0.5 - band) <= g <=
    floor(v + 0.5 + band): exactly rint(v), unless v lies within band of a .5 tie, where either neighbour is accepted.
    Returns (bad, excused, used): bytes outside the rule, bytes within band of a tie, bytes that differ from rint(v)."""
    v = np.asarray(v, np.float64)
    g = np.asarray(g).astype(np.int64)
    lo, hi = np.floor(v + 0.5 - band), np.floor(v + 0.5 + band)
    return (g < lo) | (g > hi), lo != hi, g != np.rint(v)


def rint_div(s, n):
    """rint(s / n) for non-negative integer arrays s and an integer n > 0, in integers: ties go to the even neighbour."""
    s = np.asarray(s, np.int64)
    q, r = s // n, s % n
    return q + ((2 * r > n) | ((2 * r == n) & (q % 2 == 1)))


def warp_halves_exact(img, sx2, sy2):
    """The bilinear zero-border warp for source coordinates that are integers or half-integers, given DOUBLED as integer arrays
    (sx2 = 2 sx): in integer arithmetic throughout.  Every weight is 0, 1/2 or 1, so 4 v is an integer sum of taps and the byte
    is rint_div(4 v, 4), ties half to even; absent taps count as 0.  Returns (bytes shaped like img, valid)."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    sx2, sy2 = np.asarray(sx2, np.int64), np.asarray(sy2, np.int64)
    x0, y0, ax, ay = sx2 // 2, sy2 // 2, (sx2 % 2)[..., None], (sy2 % 2)[..., None]     # floor; weight of the far tap in halves
    src = img.astype(np.int64).reshape(h, w, -1)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * ok[..., None]

    top = tap(y0, x0) * (2 - ax) + tap(y0, x0 + 1) * ax
    bot = tap(y0 + 1, x0) * (2 - ax) + tap(y0 + 1, x0 + 1) * ax
    v4 = top * (2 - ay) + bot * ay
    valid = (sx2 > -2) & (sx2 < 2 * w) & (sy2 > -2) & (sy2 < 2 * h)
    return rint_div(v4, 4).astype(np.uint8).reshape(img.shape), valid


def nearest_halves_exact(img, sx2, sy2):
    """The nearest-neighbour warp for doubled integer source coordinates: a half-integer goes to its EVEN neighbour (rint)."""
    img = np.asarray(img)
    h, w = img.shape[:2]

    def near(s2):
        s2 = np.asarray(s2, np.int64)
        lo = s2 // 2
        return np.where(s2 % 2 == 0, lo, lo + (lo % 2))
    rx, ry = near(sx2), near(sy2)
    inside = (rx >= 0) & (rx < w) & (ry >= 0) & (ry < h)
    src = img.reshape(h, w, -1)
    out = src[np.clip(ry, 0, h - 1), np.clip(rx, 0, w - 1)] * inside[..., None].astype(img.dtype)
    return out.reshape(img.shape), inside


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


# ---- correlation lookup ---------------------------------------------------------------------------------------------------------
# What one fp32 bilinear sample of the lookup kernels can lie from the fp64 value, per unit of M = the largest |tap| of its
# four.  The kernels compute fx = xs - floor(xs) exactly (xs = x * 2^-l is exact and |xs| < 2^23), so what remains are the
# roundings of three lerps q0 * (1 - w) + q1 * w: 1 - w, two products and a sum each, the second-stage operands carrying the
# first stage's error.  A CPU restatement of that arithmetic (tests/test_lookup_edges_cpu.py) measured at most 3.8 units of
# 2^-24 M; the constant is twice the measured maximum, rounded up to a power of two (profiles/README.md records both).
LOOKUP_BAND = 8 * 2.0 ** -24
LOOKUP_FAR = 1.0e6                   # a coordinate beyond this at its level (or not finite) is "nowhere": value 0


def lookup64(planes, coords, radius):
    """The multi-scale correlation lookup in pixel coordinates, float64: planes[l] (P, H_l, W_l) (independent inputs, any
    sizes), coords (P, 2) = (x, y) -> (value, M), both (P, L (2r+1)^2).  For level l and window element (i, j): xs = x / 2^l +
    (i - r), ys = y / 2^l + (j - r), x0 = floor(xs), fx = xs - x0 (same for y), the four taps (x0 | x0 + 1, y0 | y0 + 1) with
    zero outside [0, W_l) x [0, H_l); channel l (2r+1)^2 + i (2r+1) + j (x-major).  M is the largest |tap| of the four.  A
    coordinate that is not finite or beyond LOOKUP_FAR at its level reads nothing: value 0, M 0."""
    c = np.asarray(coords, np.float64)
    P, n = len(c), 2 * radius + 1
    vals, mags = [], []
    for l, pl in enumerate(planes):
        pl = np.asarray(pl, np.float64)
        assert pl.shape[0] == P
        H, W = pl.shape[1:]
        x, y = c[:, 0] / 2.0 ** l, c[:, 1] / 2.0 ** l
        with np.errstate(invalid="ignore"):            # (NaN compares false without this on current numpy; older ones warned)
            live = (np.abs(x) <= LOOKUP_FAR) & (np.abs(y) <= LOOKUP_FAR)
        xl, yl = np.where(live, x, 0.0), np.where(live, y, 0.0)
        x0, y0 = np.floor(xl), np.floor(yl)
        fx, fy = (xl - x0)[:, None, None], (yl - y0)[:, None, None]
        xs = x0.astype(np.int64)[:, None] - radius + np.arange(n + 1)[None]
        ys = y0.astype(np.int64)[:, None] - radius + np.arange(n + 1)[None]
        ok = ((ys >= 0) & (ys < H))[:, :, None] & ((xs >= 0) & (xs < W))[:, None, :] & live[:, None, None]
        patch = pl[np.arange(P)[:, None, None], np.clip(ys, 0, H - 1)[:, :, None], np.clip(xs, 0, W - 1)[:, None, :]] * ok
        tl, tr, bl, br = patch[:, :n, :n], patch[:, :n, 1:], patch[:, 1:, :n], patch[:, 1:, 1:]       # [P, j (y), i (x)]
        v = (tl * (1 - fx) + tr * fx) * (1 - fy) + (bl * (1 - fx) + br * fx) * fy
        m = np.maximum(np.maximum(np.abs(tl), np.abs(tr)), np.maximum(np.abs(bl), np.abs(br)))
        vals.append(v.transpose(0, 2, 1).reshape(P, n * n))                                       # -> [P, i, j]
        mags.append(m.transpose(0, 2, 1).reshape(P, n * n))
    return np.concatenate(vals, 1), np.concatenate(mags, 1)


# ---- flow-head gather -----------------------------------------------------------------------------------------------------------
def flow_head_gather64(part, n_planes, hf, wf, bias=None):
    """delta[p, o] = bias[o] + sum over the 9 taps (ky, kx) and the planes of part[plane P + q, (3 ky + kx) 2 + o], q the
    neighbour (y + ky - 1, x + kx - 1) of p, taps outside the grid zero; float64.  part (>= n_planes P, >= 18), P = hf wf.
    Returns (delta (P, 2), sum of the absolute terms (P, 2)): a fixed-order fp32 sum of n terms lies within n 2^-24 times the
    latter of the former (gather_band)."""
    P = hf * wf
    pt = np.asarray(part, np.float64)[:n_planes * P, :18].reshape(n_planes, hf, wf, 9, 2)
    b = np.zeros(2) if bias is None else np.asarray(bias, np.float64).reshape(-1)[:2]
    pad = np.zeros((n_planes, hf + 2, wf + 2, 9, 2))
    pad[:, 1:-1, 1:-1] = pt
    delta, mag = np.zeros((hf, wf, 2)) + b, np.zeros((hf, wf, 2)) + np.abs(b)
    for ky in range(3):
        for kx in range(3):
            t = pad[:, ky:ky + hf, kx:kx + wf, 3 * ky + kx]
            delta += t.sum(0)
            mag += np.abs(t).sum(0)
    return delta.reshape(P, 2), mag.reshape(P, 2)


def gather_band(n_planes, mag):
    """The standard bound of a fixed-order fp32 sum: (number of additions + 1) 2^-24 sum |terms|; the kernels add 9 n_planes
    terms to the bias (n_planes - 1 additions per tap, then 9 onto the running sum)."""
    return (9 * n_planes + 1) * U32 * np.asarray(mag, np.float64)


# ---- convex upsampling ----------------------------------------------------------------------------------------------------------
# fp32 softmax over 9 logits and a 9-term weighted sum: exp of a difference (one rounding in the difference, about one unit in
# expf), the denominator's 8 additions, a division and a product per tap, 8 additions of terms bounded by max |8 v_k|: below
# 32 units of 2^-24 max |8 v_k| (the CPU restatement in tests/test_lookup_edges_cpu.py stays inside it with zero violations).
CONVEX_BAND = 32 * 2.0 ** -24


def convex_upsample64(values, mask, hf, wf):
    """out[c, 8 hc + i, 8 wc + j] = sum_k softmax_k(mask[p, k 64 + 8 i + j]) 8 values[c, q_k], q_k the neighbour (hc + k // 3 -
    1, wc + k % 3 - 1) of cell p = (hc, wc), zero outside the grid; float64.  values (C, hf wf), mask (hf wf, >= 576) ->
    (out (C, 8 hf, 8 wf), M (C, 8 hf, 8 wf) = max_k |8 values[c, q_k]| per output)."""
    v = np.asarray(values, np.float64)
    C = v.shape[0]
    m = np.asarray(mask, np.float64)[:, :576].reshape(hf, wf, 9, 8, 8)
    e = np.exp(m - m.max(2, keepdims=True))
    s = e / e.sum(2, keepdims=True)                                         # (hf, wf, 9, 8, 8)
    pad = np.zeros((C, hf + 2, wf + 2))
    pad[:, 1:-1, 1:-1] = 8.0 * v.reshape(C, hf, wf)
    out, mag = np.zeros((C, hf, wf, 8, 8)), np.zeros((C, hf, wf, 8, 8))
    for k in range(9):
        nb = pad[:, k // 3:k // 3 + hf, k % 3:k % 3 + wf][..., None, None]
        out += s[None, :, :, k] * nb
        mag = np.maximum(mag, np.abs(nb))
    tr = lambda a: a.transpose(0, 1, 3, 2, 4).reshape(C, 8 * hf, 8 * wf)    # noqa: E731
    return tr(out), tr(mag)
