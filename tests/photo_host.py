"""The photometric refinement restated in plain numpy, step by step as the section states it, with a dtype
switch: float64 is the reference the kernels are compared with, float32 the yardstick that says how far two correct
implementations of different precision lie apart.  Also the seeded cases of tests/test_photo_cpu.py and tests/test_photo_gpu.py."""
import math
from types import SimpleNamespace

import numpy as np

STATUS = ("CONVERGED", "MAX_ITERS", "TOO_FEW", "SINGULAR", "NONFINITE")
DEFAULTS = dict(iters=10, gain_bias=True, huber_k=None, stride=1, min_valid=0.5, eps=1e-3)


def intensity(img, dtype=np.float64):
    """S = c0 + c1 + c2 of an (h, w, 3) image."""
    a = np.asarray(img).astype(dtype)
    return (a[..., 0] + a[..., 1]) + a[..., 2]


def problem(template, mask, stride=1, weights=None, dtype=np.float64):
    """The fixed part: the box, the normalisation, the pixel set Omega and its template values and gradients."""
    T = intensity(template, dtype)
    h, w = T.shape
    mask = np.asarray(mask)
    ys, xs = np.nonzero(mask > 0)
    P = SimpleNamespace(h=h, w=w, stride=int(stride), dtype=dtype, empty=len(xs) == 0, n_set=0)
    if P.empty:
        return P
    x0, x1, y0, y1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
    keep = (xs >= 1) & (xs <= w - 2) & (ys >= 1) & (ys <= h - 2) & ((xs - x0) % stride == 0) & ((ys - y0) % stride == 0)
    xs, ys = xs[keep], ys[keep]
    P.box = (x0, y0, x1, y1)
    P.cx, P.cy, P.s = dtype((x0 + x1) / 2.0), dtype((y0 + y1) / 2.0), dtype(max(x1 - x0, y1 - y0, 1) / 2.0)
    P.xs, P.ys, P.n_set = xs, ys, len(xs)
    P.T = T[ys, xs]
    half = dtype(0.5)
    P.gx = P.s * ((T[ys, xs + 1] - T[ys, xs - 1]) * half)
    P.gy = P.s * ((T[ys + 1, xs] - T[ys - 1, xs]) * half)
    P.xn = (xs.astype(dtype) - P.cx) / P.s
    P.yn = (ys.astype(dtype) - P.cy) / P.s
    P.weight = np.ones(len(xs), dtype) if weights is None else np.asarray(weights)[ys, xs].astype(dtype)
    return P


def to_state(P, W):
    """M = W N^-1, N: (x, y) -> ((x - cx) / s, (y - cy) / s)."""
    W = np.asarray(W, P.dtype)
    Ninv = np.array([[P.s, 0, P.cx], [0, P.s, P.cy], [0, 0, 1]], P.dtype)
    return W @ Ninv


def from_state(P, M):
    """W = M N / h33."""
    N = np.array([[1 / P.s, 0, -P.cx / P.s], [0, 1 / P.s, -P.cy / P.s], [0, 0, 1]], P.dtype)
    W = M @ N
    return W / W[2, 2]


def evaluate(P, SF, M, g, b, gain_bias=True, huber_k=None):
    """The sums at a state: SF the frame's intensity (hf, wf) in P.dtype.  -> G, r, cs = sum weight rho, ws = sum weight, n, the
    magnitudes of the test's bound (the per-pixel terms with e replaced by |I| + |g T| + |b| and every factor by its modulus) and
    the smallest distance of a coordinate from a validity bound."""
    dt = P.dtype
    hf, wf = SF.shape
    g, b = dt(g), dt(b)
    with np.errstate(all="ignore"):
        qx = M[0, 0] * P.xn + M[0, 1] * P.yn + M[0, 2]
        qy = M[1, 0] * P.xn + M[1, 1] * P.yn + M[1, 2]
        qz = M[2, 0] * P.xn + M[2, 1] * P.yn + M[2, 2]
        u, v = qx / qz, qy / qz
        valid = (qz > 0) & (u >= 0) & (u < wf - 1) & (v >= 0) & (v < hf - 1)
        front = qz > 0
        margin = np.inf
        if front.any():
            margin = float(min(np.abs(u[front]).min(), np.abs(u[front] - (wf - 1)).min(), np.abs(v[front]).min(),
                               np.abs(v[front] - (hf - 1)).min()))
    u, v = u[valid], v[valid]
    xn, yn, T, gx, gy, wt = P.xn[valid], P.yn[valid], P.T[valid], P.gx[valid], P.gy[valid], P.weight[valid]
    fu, fv = np.floor(u), np.floor(v)
    fx, fy = u - fu, v - fv
    iu, iv = fu.astype(np.int64), fv.astype(np.int64)
    one = dt(1)
    I = (one - fy) * ((one - fx) * SF[iv, iu] + fx * SF[iv, iu + 1]) + fy * ((one - fx) * SF[iv + 1, iu] + fx * SF[iv + 1, iu + 1])
    e = I - g * T - b
    E = np.abs(I) + np.abs(g * T) + np.abs(b)
    ae = np.abs(e)
    om, rho, mrho = wt.copy(), e * e, E * E
    if huber_k is not None:
        k = dt(3.0 * huber_k)
        out = ae > k
        with np.errstate(all="ignore"):
            om = np.where(out, wt * (k / ae), wt)
        rho = np.where(out, dt(2) * k * ae - k * k, rho)
        mrho = np.where(out, dt(2) * k * E + k * k, mrho)
    d = gx * xn + gy * yn
    cols = [g * (gx * xn), g * (gx * yn), g * gx, g * (gy * xn), g * (gy * yn), g * gy, g * (-xn * d), g * (-yn * d)]
    if gain_bias:
        cols += [T, np.ones_like(T)]
    A = np.stack(cols, 1) if len(T) else np.zeros((0, len(cols)), dt)
    oA = om[:, None] * A
    out = SimpleNamespace(G=oA.T @ A, r=oA.T @ e, cs=(wt * rho).sum(dtype=dt), ws=wt.sum(dtype=dt), n=int(valid.sum()), margin=margin)
    aA = np.abs(oA).astype(np.float64)
    out.mag_G = aA.T @ np.abs(A).astype(np.float64)
    out.mag_r = aA.T @ E.astype(np.float64)
    out.mag_cs = float((wt * mrho).sum(dtype=np.float64))
    out.mag_ws = float(wt.sum(dtype=np.float64))
    return out


def cholesky_solve(G, r):
    """G delta = r by Cholesky without a ridge -> delta, or None: a pivot that is not finite or <= 2^-40 of its diagonal entry."""
    dt = G.dtype.type
    n = len(r)
    L = np.zeros((n, n), dt)
    for j in range(n):
        for i in range(j, n):
            v = G[j, i]
            for q in range(j):
                v = v - L[i, q] * L[j, q]
            if i == j:
                if not np.isfinite(v) or not (v > G[j, j] * dt(2.0 ** -40)):
                    return None
                L[j, j] = np.sqrt(v)
            else:
                L[i, j] = v / L[j, j]
    y = np.zeros(n, dt)
    for i in range(n):
        v = r[i]
        for q in range(i):
            v = v - L[i, q] * y[q]
        y[i] = v / L[i, i]
    x = np.zeros(n, dt)
    for i in range(n - 1, -1, -1):
        v = y[i]
        for q in range(i + 1, n):
            v = v - L[q, i] * x[q]
        x[i] = v / L[i, i]
    return x if np.all(np.isfinite(x)) else None


def project(M, pts):
    q = np.asarray(M, np.float64) @ np.concatenate([np.asarray(pts, np.float64), np.ones((len(pts), 1))], 1).T
    return (q[:2] / q[2]).T


def box_corners(box):
    x0, y0, x1, y1 = box
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)


def corner_distance(box, Ha, Hb):
    """The largest distance, in frame pixels, between the images of the box's four corners under two homographies."""
    c = box_corners(box)
    return float(np.sqrt(((project(Ha, c) - project(Hb, c)) ** 2).sum(1)).max())


def refine(template, mask, frame, W0, iters=10, gain_bias=True, huber_k=None, stride=1, min_valid=0.5, eps=1e-3, weights=None,
           dtype=np.float64):
    """-> SimpleNamespace(H, status, best, H_iter, gain, bias, cost, n_valid, step, rms_before, rms_after, margin, launched)."""
    P = problem(template, mask, stride, weights, dtype)
    nu = 10 if gain_bias else 8
    W0 = np.asarray(W0, np.float64)
    R = SimpleNamespace(H=W0.copy(), status="TOO_FEW", best=-1, H_iter=[], gain=[], bias=[], cost=[], n_valid=[], step=[],
                        rms_before=float("nan"), rms_after=float("nan"), margin=np.inf, launched=False, n_set=P.n_set, evals=[])
    if P.empty or P.n_set < nu:
        return _finish(R)
    R.launched = True
    SF = intensity(frame, dtype)
    n_need = max(nu, int(math.ceil(min_valid * P.n_set)))
    M, g, b = to_state(P, W0), dtype(1), dtype(0)
    nc = (box_corners(P.box) - [float(P.cx), float(P.cy)]) / float(P.s)
    best_cost, conv_at = None, -1
    for k in range(iters + 1):
        ev = evaluate(P, SF, M, g, b, gain_bias, huber_k)
        with np.errstate(all="ignore"):
            cost = np.sqrt(ev.cs / ev.ws) / dtype(3)
        W = from_state(P, M)
        R.H_iter.append(np.asarray(W, np.float64)), R.gain.append(float(g)), R.bias.append(float(b / dtype(3)))
        R.cost.append(float(cost)), R.n_valid.append(ev.n), R.step.append(float("nan"))
        R.margin = min(R.margin, ev.margin)
        R.evals.append(ev)
        if ev.n < n_need or not (ev.ws > 0):
            R.status = "TOO_FEW"
            break
        if not (np.isfinite(cost) and np.all(np.isfinite(ev.G)) and np.all(np.isfinite(ev.r))):
            R.status = "NONFINITE"
            break
        if best_cost is None or cost < best_cost:
            R.best, best_cost = k, cost
        if k == iters:
            R.status = "MAX_ITERS"
            break
        if k == conv_at:
            R.status = "CONVERGED"
            break
        delta = cholesky_solve(ev.G, ev.r)
        if delta is None:
            R.status = "SINGULAR"
            break
        D = np.eye(3, dtype=dtype) + np.array([[delta[0], delta[1], delta[2]], [delta[3], delta[4], delta[5]],
                                               [delta[6], delta[7], 0]], dtype)
        M1 = (M @ np.linalg.inv(D)).astype(dtype)
        if gain_bias:
            g, b = g + delta[8], b + delta[9]
        step = float(np.sqrt(((project(M1, nc) - project(M, nc)) ** 2).sum(1)).max())
        R.step[-1] = step
        M = M1
        if step < eps:
            conv_at = k + 1
    return _finish(R)


def _finish(R):
    if R.best >= 0:
        R.H = R.H_iter[R.best]
        R.rms_after = R.cost[R.best]
    if R.cost:
        R.rms_before = R.cost[0]
    for name in ("H_iter", "gain", "bias", "cost", "n_valid", "step"):
        v = getattr(R, name)
        setattr(R, name, np.asarray(v, np.float64 if name != "n_valid" else np.int64).reshape((len(v), 3, 3) if name == "H_iter"
                                                                                               else (len(v),)))
    return R


# ---- the seeded cases ---------------------------------------------------------------------------------------------------------
TEMPLATE_HW, FRAME_HW = (64, 96), (72, 104)
GAIN, BIAS = 1.12, -9.0
SEEDS = (11, 12, 13)          # (chosen so that test_photo_cpu.test_boundary_margins holds; change a seed, never the margin)


def base_template():
    from woft_amd import synth
    return synth.make_template(TEMPLATE_HW[0], TEMPLATE_HW[1], seq_id=3)


def base_mask():
    m = np.zeros(TEMPLATE_HW, np.uint8)
    m[12:52, 20:77] = 255
    m[12:20, 20:30] = 0
    return m


BOX = (20, 12, 76, 51)


def render_frame(template, H, gain=GAIN, bias=BIAS, out_hw=FRAME_HW):
    import hsynth_host
    out, _ = hsynth_host.render(template, H, gain=gain, bias=bias, out_hw=out_hw)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def base_case(seed, shift=(0.0, 0.0), nudge=(0.0, 0.0)):
    """-> (template, mask, frame, H_gt, W0): H_gt moves the box's corners by up to 4 px (then by `shift`), W0 is H_gt with the
    projected corners moved by up to 1.5 px (then by `nudge`)."""
    from woft_amd.hsynth import homography_from_4pts
    rs = np.random.RandomState(seed)
    template, mask = base_template(), base_mask()
    c = box_corners(BOX)
    H_gt = homography_from_4pts(c, c + rs.uniform(-4.0, 4.0, (4, 2)) + np.asarray(shift))
    frame = render_frame(template, H_gt)
    W0 = homography_from_4pts(c, project(H_gt, c) + rs.uniform(-1.5, 1.5, (4, 2)) + np.asarray(nudge))
    return template, mask, frame, H_gt, W0


CONFIGS = {"l2": dict(gain_bias=True, huber_k=None), "huber6": dict(gain_bias=True, huber_k=6.0)}
PARTIAL_SHIFT = (-35.0, 0.0)        # a quarter of the mask's columns leave the frame on the left


def partial_case():
    """Part of the mask lies outside the frame: n_valid changes between iterates and stays above half of n_set."""
    return base_case(SEEDS[0], shift=PARTIAL_SHIFT)


def shrinking_case():
    """The partial case started one and a half pixels too far inside: the steps move pixels out of the frame, and with min_valid =
    n_0 / n_set a later iterate falls below the threshold.  -> (template, mask, frame, H_gt, W0, min_valid)."""
    template, mask, frame, H_gt, W0 = base_case(SEEDS[0], shift=PARTIAL_SHIFT, nudge=(1.5, 0.0))
    r = refine(template, mask, frame, W0, iters=0)
    return template, mask, frame, H_gt, W0, float(r.n_valid[0]) / r.n_set


def outside_W0():
    return np.array([[1.0, 0.0, 500.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def eval_tolerances(ev, hf, wf):
    """The bound of the single evaluation: (n_valid + 64 + 8 max(hf, wf)) 2^-53 times the summed magnitudes."""
    f = (ev.n + 64 + 8 * max(hf, wf)) * 2.0 ** -53
    return SimpleNamespace(G=f * ev.mag_G, r=f * ev.mag_r, cs=f * ev.mag_cs, ws=f * ev.mag_ws)


def cost_tolerance(ev, hf, wf):
    """The evaluation bound carried to the reported cost c = sqrt(cs / ws) / 3: 18 c dc = d(cs / ws) <= tol(cs) / ws +
    cs tol(ws) / ws^2."""
    t = eval_tolerances(ev, hf, wf)
    cs, ws = float(ev.cs), float(ev.ws)
    return (t.cs / ws + cs * t.ws / ws ** 2) / (18.0 * math.sqrt(cs / ws) / 3.0)
