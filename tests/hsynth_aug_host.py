"""float64 numpy restatement of woft_hsynth_render_bg and woft_hsynth_augment, written from the semantics in include/woft_hip.h
(DESIGN.md section 24), on top of tests/hsynth_host.py: the background composite, the blur with replicate border, the affine
colour map and the noise, whose integer part is done in uint32 arithmetic exactly.  Plus the fixed cases the CPU and the GPU
tests share."""
import numpy as np

import hsynth_host as hh

Z_SCALE = np.float32(np.sqrt(3.0) / 65536.0)       # the kernel's one constant, rounded to float32 as it is there
Z_MAX = 3.47


# ---- background ----------------------------------------------------------------------------------------------------------------
def _bilinear_replicate(planes, sx, sy):
    """Replicate-border bilinear sample of planes (h, w, C) float64 at (sx, sy) -> (..., C); every tap counts, at its clamped
    index.  The caller masks non-finite coordinates."""
    h, w = planes.shape[:2]
    fx0, fy0 = np.floor(sx), np.floor(sy)
    fx, fy = (sx - fx0)[..., None], (sy - fy0)[..., None]
    x0 = np.clip(fx0, -4, w + 4).astype(np.int64)
    y0 = np.clip(fy0, -4, h + 4).astype(np.int64)

    def tap(yy, xx):
        return planes[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
    top = tap(y0, x0) * (1 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (1 - fx) + tap(y0 + 1, x0 + 1) * fx
    return top * (1 - fy) + bot * fy


def background_at(bg, H_bg, out_hw):
    """g (h, w, 3): the background (hb, wb, 3) uint8 seen through H_bg (background -> destination); 0 where the denominator is not
    positive or a coordinate is not finite."""
    h, w = out_hw
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    gx, gy, d = hh._source(np.linalg.inv(np.asarray(H_bg, np.float64)), xs, ys)
    with np.errstate(invalid="ignore"):
        ok = (d > 0) & np.isfinite(gx) & np.isfinite(gy)
    g = _bilinear_replicate(bg.astype(np.float64), np.where(ok, gx, 0.0), np.where(ok, gy, 0.0))
    return g * ok[..., None]


def plane_coverage(src_hw, H_gt, out_hw):
    """P (h, w): the bilinear interpolation of the base image's in-image flags; 0 where the denominator is not positive."""
    h, w = out_hw
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    sx, sy, d = hh._source(np.linalg.inv(np.asarray(H_gt, np.float64)), xs, ys)
    P = hh._bilinear(np.ones(tuple(src_hw) + (1,)), sx, sy)[..., 0]
    with np.errstate(invalid="ignore"):
        return np.where(d > 0, P, 0.0)


def render_bg(base, H_gt, bg, H_bg, occluders=(), gain=None, bias=None, out_hw=None):
    """-> (out_f64 (h, w, 3) un-rounded, cover (h, w), plane (h, w)): hsynth_host.render's steps with v + (1 - P) g before the
    gain."""
    h, w = base.shape[:2] if out_hw is None else out_hw
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    sx, sy, _ = hh._source(np.linalg.inv(np.asarray(H_gt, np.float64)), xs, ys)
    v = hh._bilinear(base.astype(np.float64), sx, sy)
    P = plane_coverage(base.shape[:2], H_gt, (h, w))
    v = v + (1 - P)[..., None] * background_at(bg, H_bg, (h, w))
    g = np.ones(3) if gain is None else np.broadcast_to(np.asarray(gain, np.float64).ravel(), (3,))
    b = np.zeros(3) if bias is None else np.broadcast_to(np.asarray(bias, np.float64).ravel(), (3,))
    v = g * v + b
    keep = np.ones((h, w))
    for tex, H_occ in occluders:
        ox, oy, _ = hh._source(np.linalg.inv(np.asarray(H_occ, np.float64)), xs, ys)
        s = hh._bilinear(hh._premultiplied(tex), ox, oy)
        A = s[..., 3]
        v = (1 - A)[..., None] * v + s[..., :3]
        keep = keep * (1 - A)
    return v, 1 - keep, P


# ---- augmentation --------------------------------------------------------------------------------------------------------------
def _mix(v):
    v = v.astype(np.uint32)
    with np.errstate(over="ignore"):
        v = v ^ (v >> np.uint32(16))
        v = v * np.uint32(0x7FEB352D)
        v = v ^ (v >> np.uint32(15))
        v = v * np.uint32(0x846CA68B)
        v = v ^ (v >> np.uint32(16))
    return v


def noise_int(seed, idx):
    """S - 131070 of the definition, int64, for the uint32 indices idx: exact."""
    idx = np.asarray(idx, dtype=np.uint64).astype(np.uint32)
    with np.errstate(over="ignore"):
        a = _mix(np.uint32(seed) ^ _mix(idx))
        b = _mix(a + np.uint32(0x9E3779B9))
    S = (a & np.uint32(0xFFFF)).astype(np.int64) + (a >> np.uint32(16)).astype(np.int64) \
        + (b & np.uint32(0xFFFF)).astype(np.int64) + (b >> np.uint32(16)).astype(np.int64)
    return S - 131070


def noise_z(seed, h, w):
    """z (h, w, 3) float64 of every pixel and channel of an (h, w) frame: idx = (y * w + x) * 3 + c modulo 2^32."""
    idx = (np.arange(h * w * 3, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).reshape(h, w, 3)
    return noise_int(seed, idx).astype(np.float64) * np.float64(Z_SCALE)


def blur(frame, taps):
    """Separable blur of frame (h, w, 3) float64 with the 2 r + 1 taps, replicate border: rows first, then columns."""
    taps = np.asarray(taps, np.float64)
    r = (len(taps) - 1) // 2
    if r == 0:
        return frame.copy()
    h, w = frame.shape[:2]
    xi = np.clip(np.arange(w)[:, None] + np.arange(-r, r + 1)[None, :], 0, w - 1)       # (w, 2r+1)
    yi = np.clip(np.arange(h)[:, None] + np.arange(-r, r + 1)[None, :], 0, h - 1)
    rows = np.einsum("ywkc,k->ywc", frame[:, xi], taps)
    return np.einsum("ykwc,k->ywc", rows[yi], taps)


def augment(frame, taps=None, colour=None, noise_sigma=0.0, seed=0, detail=False):
    """frame (h, w, 3) float -> u (h, w, 3) float64 un-rounded; taps and colour as the entry takes them (float32 values, used as
    the numbers they are).  detail: also the largest magnitude among the restatement's intermediate values -- the input, the
    blurred frame, the offset, every product M_cj t_j, their absolute sum per channel, the result before and after the noise."""
    f = np.asarray(frame, np.float64)
    h, w = f.shape[:2]
    t = f if taps is None else blur(f, taps)
    mag = max(float(np.abs(f).max()), float(np.abs(t).max()))
    u = t
    if colour is not None:
        c = np.asarray(colour, np.float64)
        M, o = c[:9].reshape(3, 3), c[9:]
        u = o + t @ M.T
        mag = max(mag, float(np.abs(o).max()), float((np.abs(t) @ np.abs(M).T + np.abs(o)).max()), float(np.abs(u).max()))
    if noise_sigma != 0.0:
        u = u + np.float64(np.float32(noise_sigma)) * noise_z(seed, h, w)
        mag = max(mag, float(np.abs(u).max()))
    return (u, mag) if detail else u


def augment_tol(radius, mag, noise_sigma):
    """(2 (2 r + 1) + 10) * 2^-24 * max(255, mag) + 2^-24 * noise_sigma * 3.47.  Each blur pass is a sum of 2 r + 1 products of
    positive taps that add up to 1: the products' roundings together stay within 2^-24 of the largest value and each of the 2 r
    adds within 2^-24 of a partial sum below it -- 2 r + 1 per pass, carried through the second pass with weight 1, through the
    colour map with at most the absolute sum mag covers.  The colour map is 3 products and 3 adds, the noise a product and an
    add, the conversion of the integer to float is exact: 8 of the 10, each within 2^-24 of an intermediate value.  z's own
    product with the float32 constant rounds once: 2^-24 |z| noise_sigma."""
    return (2 * (2 * radius + 1) + 10) * 2.0 ** -24 * max(255.0, mag) + 2.0 ** -24 * noise_sigma * Z_MAX


def to_u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ---- the fixed cases of tests/test_hsynth_aug_gpu.py ---------------------------------------------------------------------------
AUG_HWS = hh.DST_HWS + ((40, 72),)      # 40 x 72: two 32 x 32 tiles and a partial one across, one and a partial one down
RADII = (0, 1, 7)
SIGMA_OF_RADIUS = {0: 0.0, 1: 0.3, 7: 2.5}       # blur_taps(sigma) has this radius


def backgrounds():
    """A 1x1 and an 11x7 background."""
    rs = np.random.RandomState(hh.CASE_SEED + 7)
    return {"1x1": np.array([[[37, 180, 220]]], np.uint8), "11x7": rs.randint(0, 256, (11, 7, 3)).astype(np.uint8)}


def background_H(bg, out_hw):
    """background -> destination: the background stretched over the frame, turned a little and bent, so that taps clamp at some
    borders and interpolate elsewhere."""
    hb, wb = bg.shape[:2]
    h, w = out_hw
    fit = np.diag([max(w - 1, 1) / max(wb - 1.0, 1.0), max(h - 1, 1) / max(hb - 1.0, 1.0), 1.0])
    bend = np.array([[0.96, 0.07, 0.4], [-0.05, 1.03, -0.3], [0.0008, -0.0005, 1.0]])
    return bend @ fit


def float_frame(out_hw, seed=0):
    """A float32 frame with values a rendered frame has, some beyond 0 .. 255."""
    rs = np.random.RandomState(hh.CASE_SEED + 11 + seed)
    return rs.uniform(-20.0, 290.0, tuple(out_hw) + (3,)).astype(np.float32)
