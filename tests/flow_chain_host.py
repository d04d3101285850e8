"""numpy restatements of csrc/flow_chain.hip (test infrastructure).

  * sample_ref32: the reference's bilinear_interpolate_torch (utils/interpolation.py:92-133) in fp32, in its operation order --
    every product and sum rounded on its own; bit-equal to the reference's CPU result (tests/golden/flow_interp.npz).
  * sample_edge64 / chain64 / fb64: the edge-exact sampler, the chain and the forward-backward check in fp64, from fp32 inputs,
    with q = pixel + flow formed in fp32 (so that validity is decided on the very numbers the kernel decides it on).
  * make_fields: the fixed recipe of the chain / fb test fields.
"""
import numpy as np

F32 = np.float32


def _clamp32(v, hi):
    """v forced into [0, hi] the way the kernel does it: NaN -> 0, +inf -> hi, -inf -> 0 (two ordered compares)."""
    lo = np.where(v >= 0, v, F32(0)).astype(F32)
    return np.where(lo <= hi, lo, F32(hi)).astype(F32)


def sample_ref32(data, x, y):
    """(C, H, W) fp32, (N,), (N,) -> (C, N) fp32: ((wa*a + wb*b) + wc*c) + wd*d with the weights from the clamped corners."""
    data, x, y = np.asarray(data, F32), np.asarray(x, F32), np.asarray(y, F32)
    _, h, w = data.shape
    with np.errstate(all="ignore"):
        fx, fy = np.floor(x), np.floor(y)
        x0, x1 = _clamp32(fx, F32(w - 1)), _clamp32(fx + F32(1), F32(w - 1))
        y0, y1 = _clamp32(fy, F32(h - 1)), _clamp32(fy + F32(1), F32(h - 1))
        ix0, ix1, iy0, iy1 = x0.astype(np.int64), x1.astype(np.int64), y0.astype(np.int64), y1.astype(np.int64)
        a, b, c, d = data[:, iy0, ix0], data[:, iy1, ix0], data[:, iy0, ix1], data[:, iy1, ix1]
        wa = ((x1 - x) * (y1 - y)).astype(F32)[None]
        wb = ((x1 - x) * (y - y0)).astype(F32)[None]
        wc = ((x - x0) * (y1 - y)).astype(F32)[None]
        wd = ((x - x0) * (y - y0)).astype(F32)[None]
        r = ((wa * a).astype(F32) + (wb * b).astype(F32)).astype(F32)
        r = (r + (wc * c).astype(F32)).astype(F32)
        r = (r + (wd * d).astype(F32)).astype(F32)
    return r


def landing32(flow):
    """(2, H, W) fp32 -> (qx, qy fp32 (H, W), valid bool): q = pixel + flow in fp32; valid iff inside the closed frame."""
    flow = np.asarray(flow, F32)
    _, h, w = flow.shape
    ys, xs = np.mgrid[:h, :w]
    with np.errstate(all="ignore"):
        qx = (xs.astype(F32) + flow[0]).astype(F32)
        qy = (ys.astype(F32) + flow[1]).astype(F32)
        valid = (qx >= 0) & (qx <= F32(w - 1)) & (qy >= 0) & (qy <= F32(h - 1))
    return qx, qy, valid


def sample_edge64(f, qx, qy, valid):
    """Edge-exact bilinear sample of the (2, H, W) field f at the valid points -> (s (2, H, W) fp64 (0 where invalid),
    tapmax (H, W): the largest |tap| of the pixel over both planes)."""
    f = np.asarray(f, F32).astype(np.float64)
    _, h, w = f.shape
    qx = np.where(valid, qx, 0).astype(np.float64)
    qy = np.where(valid, qy, 0).astype(np.float64)
    x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = qx - x0, qy - y0
    d00, d01, d10, d11 = f[:, y0, x0], f[:, y0, x1], f[:, y1, x0], f[:, y1, x1]
    s = (1 - ay) * ((1 - ax) * d00 + ax * d01) + ay * ((1 - ax) * d10 + ax * d11)
    tapmax = np.max(np.abs(np.stack([d00, d01, d10, d11])), axis=(0, 1))
    return np.where(valid, s, 0.0), tapmax


def chain64(fab, fbc):
    """-> (fac (2, H, W) fp64, NaN where q is invalid; valid; tapmax)."""
    qx, qy, valid = landing32(fab)
    s, tapmax = sample_edge64(fbc, qx, qy, valid)
    fac = np.where(valid, np.asarray(fab, F32).astype(np.float64) + s, np.nan)
    return fac, valid, tapmax


def fb64(fab, fba, alpha, beta):
    """-> (err (H, W) fp64, +inf where invalid; ok bool; e2; bound; valid) with alpha, beta as the fp32 values the kernel gets."""
    qx, qy, valid = landing32(fab)
    b, _ = sample_edge64(fba, qx, qy, valid)
    f = np.asarray(fab, F32).astype(np.float64)
    alpha, beta = float(F32(alpha)), float(F32(beta))
    e2 = (f[0] + b[0]) ** 2 + (f[1] + b[1]) ** 2
    bound = alpha * ((f[0] ** 2 + f[1] ** 2) + (b[0] ** 2 + b[1] ** 2)) + beta
    err = np.where(valid, np.sqrt(e2), np.inf)
    ok = valid & (e2 <= bound)
    return err, ok, e2, bound, valid


SHAPES = ((5, 7), (33, 65), (40, 72), (1, 9), (9, 1))


def make_fields(h, w, seed=0):
    """The chain / fb test fields (fixed recipe) -> (forward, backward), (2, h, w) fp32 each.  Forward: the flow of a homography
    within 5 % of the identity (relative to the frame size) plus 0.3 px Gaussian noise.  Backward: the flow of its inverse plus
    the same kind of noise and a 4 px offset on the middle ninth of the frame (pixels that fail the check in-frame)."""
    rs = np.random.RandomState(1000 + 131 * h + w + seed)
    s = float(max(h, w))
    Hm = np.eye(3)
    Hm[:2, :2] += rs.uniform(-0.05, 0.05, (2, 2))
    Hm[:2, 2] = rs.uniform(-0.05, 0.05, 2) * s
    Hm[2, :2] = rs.uniform(-0.05, 0.05, 2) / s
    ys, xs = np.mgrid[:h, :w].astype(np.float64)

    def flow_of(M):
        d = M[2, 0] * xs + M[2, 1] * ys + M[2, 2]
        return np.stack([(M[0, 0] * xs + M[0, 1] * ys + M[0, 2]) / d - xs, (M[1, 0] * xs + M[1, 1] * ys + M[1, 2]) / d - ys])
    fwd = flow_of(Hm) + rs.normal(0.0, 0.3, (2, h, w))
    bwd = flow_of(np.linalg.inv(Hm)) + rs.normal(0.0, 0.3, (2, h, w))
    bwd[:, h // 3:h - h // 3, w // 3:w - w // 3] += 4.0
    for axis, side in ((1, h), (0, w)):            # a one-row / one-column frame: any flow across it leaves the frame
        if side == 1:
            fwd[axis], bwd[axis] = 0.0, 0.0
    return fwd.astype(F32), bwd.astype(F32)
