"""Host restatement of the RANSAC estimator of woft_amd/csrc/ransac.hip (a helper of the RANSAC tests, not a conftest): the same
SplitMix64 index stream, cv2's sample check, the exact fp64 4-point model, cv2's fp32 error formula and cv2's SEQUENTIAL
selection loop (RANSACUpdateNumIters after every new best), written as plainly as possible; every fp64 / fp32 operation in the
order the kernel performs it, so that the per-hypothesis inlier counts agree exactly.  `geometric_optimum` is the fp64
Levenberg-Marquardt optimum of sum |proj(H, a) - b|^2 over an inlier set, run to convergence (the kernel stops after 10)."""
import math

import numpy as np

M64 = (1 << 64) - 1
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_MIN = float(np.finfo(np.float64).tiny)
MAX_ATTEMPTS = 1000


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_index(key, k, c, n):
    u = splitmix64(key ^ ((k << 32) | c))
    return ((u >> 32) * n) >> 32


def _collinear(pi, pj, pk):
    f = np.float32
    dx1, dy1 = float(f(pj[0]) - f(pi[0])), float(f(pj[1]) - f(pi[1]))
    dx2, dy2 = float(f(pk[0]) - f(pi[0])), float(f(pk[1]) - f(pi[1]))
    return abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dx2) + abs(dy1) + abs(dy2))


def _any_collinear(p):
    return _collinear(p[2], p[1], p[0]) or _collinear(p[3], p[1], p[0]) or _collinear(p[3], p[2], p[0]) or \
        _collinear(p[3], p[2], p[1])


def _orient(a, b, c):
    x0, y0, x1, y1, x2, y2 = float(a[0]), float(a[1]), float(b[0]), float(b[1]), float(c[0]), float(c[1])
    return x0 * (y1 - y2) - y0 * (x1 - x2) + (x1 * y2 - x2 * y1)


def check_subset(a, b):
    if _any_collinear(a) or _any_collinear(b):
        return False
    neg = 0
    for t in ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3)):
        neg += _orient(*(a[i] for i in t)) * _orient(*(b[i] for i in t)) < 0.0
    return neg in (0, 4)


def draw_sample(pa, pb, key, k):
    """-> the 4 indices of hypothesis k, or None ("no sample")."""
    n, c = pa.shape[0], 0
    for _ in range(MAX_ATTEMPTS):
        idx = []
        for _i in range(4):
            while True:
                v = draw_index(key, k, c, n)
                c += 1
                if v not in idx:
                    break
            idx.append(v)
        if check_subset(pa[idx], pb[idx]):
            return idx
    return None


def _square_to_quad(p):
    x0, y0, x1, y1, x2, y2, x3, y3 = (float(v) for v in p.reshape(-1))
    sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
    dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
    den = dx1 * dy2 - dx2 * dy1
    if den == 0.0:
        return None
    g, h = (sx * dy2 - dx2 * sy) / den, (dx1 * sy - sx * dy1) / den
    return [x1 - x0 + g * x1, x3 - x0 + h * x3, x0, y1 - y0 + g * y1, y3 - y0 + h * y3, y0, g, h, 1.0]


def model4(a, b):
    """Exact 4-point model a -> b, H = Q_b adj(Q_a) scaled to h33 = 1 (9 Python floats), or None when singular."""
    qa, qb = _square_to_quad(a), _square_to_quad(b)
    if qa is None or qb is None:
        return None
    adj = [qa[4] * qa[8] - qa[5] * qa[7], qa[2] * qa[7] - qa[1] * qa[8], qa[1] * qa[5] - qa[2] * qa[4],
           qa[5] * qa[6] - qa[3] * qa[8], qa[0] * qa[8] - qa[2] * qa[6], qa[2] * qa[3] - qa[0] * qa[5],
           qa[3] * qa[7] - qa[4] * qa[6], qa[1] * qa[6] - qa[0] * qa[7], qa[0] * qa[4] - qa[1] * qa[3]]
    H = [qb[r * 3] * adj[c] + qb[r * 3 + 1] * adj[3 + c] + qb[r * 3 + 2] * adj[6 + c] for r in range(3) for c in range(3)]
    s = H[8]
    if s == 0.0:
        return None
    H = [H[i] / s for i in range(8)] + [1.0]
    return H if all(math.isfinite(v) for v in H) else None


def errors_f32(H, pa, pb):
    """cv2's fp32 reprojection error of every point."""
    hf = np.asarray(H[:8], dtype=np.float64).astype(np.float32)
    x, y, X, Y = pa[:, 0], pa[:, 1], pb[:, 0], pb[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):     # (a point on the model's horizon: inf, as in fp32)
        ww = np.float32(1.0) / (hf[6] * x + hf[7] * y + np.float32(1.0))
        dx = (hf[0] * x + hf[1] * y + hf[2]) * ww - X
        dy = (hf[3] * x + hf[4] * y + hf[5]) * ww - Y
        return dx * dx + dy * dy


def errors_f64(H, pa, pb):
    a, b = pa.astype(np.float64), pb.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = H[6] * a[:, 0] + H[7] * a[:, 1] + 1.0
        u = (H[0] * a[:, 0] + H[1] * a[:, 1] + H[2]) / z
        v = (H[3] * a[:, 0] + H[4] * a[:, 1] + H[5]) / z
        return (u - b[:, 0]) ** 2 + (v - b[:, 1]) ** 2


def update_num_iters(p, ep, model_points, max_iters):
    """RANSACUpdateNumIters as OpenCV publishes it ((1 - ep)^4 as two squarings, as the kernel does)."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    t = 1.0 - ep
    t2 = t * t
    denom = 1.0 - t2 * t2
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else int(np.rint(num / denom))


class Hypotheses:
    """Hypothesis k of a fit: its sample, model, inlier count (-1 no sample, 0 singular) and the number of points whose fp64
    error lies within 1e-4 thr^2 of thr^2 (where an fp32 decision may legitimately differ)."""

    def __init__(self, pa, pb, thr, seed):
        self.pa, self.pb = np.ascontiguousarray(pa, np.float32), np.ascontiguousarray(pb, np.float32)
        self.thr2 = np.float32(float(thr) * float(thr))
        self.key = splitmix64(int(seed) & M64)
        self._cache = {}

    def get(self, k):
        if k not in self._cache:
            idx = draw_sample(self.pa, self.pb, self.key, k)
            H = None if idx is None else model4(self.pa[idx], self.pb[idx])
            if idx is None:
                cnt, near = -1, 0
            elif H is None:
                cnt, near = 0, 0
            else:
                cnt = int((errors_f32(H, self.pa, self.pb) <= self.thr2).sum())
                near = int((np.abs(errors_f64(H, self.pa, self.pb) - float(self.thr2)) <= 1e-4 * float(self.thr2)).sum())
            self._cache[k] = (idx, H, cnt, near)
        return self._cache[k]


def ransac_host(pa, pb, max_iters=10000, thr=1.4142, conf=0.995, seed=0):
    """cv2's sequential loop -> dict(status, best_k, iterations, n_inliers, H (best model), mask, hyp (Hypotheses))."""
    n = pa.shape[0]
    assert n >= 4
    hyp = Hypotheses(pa, pb, thr, seed)
    if n == 4:
        H = model4(hyp.pa, hyp.pb)
        ok = H is not None
        return dict(status=0 if ok else 2, best_k=0 if ok else -1, iterations=0, n_inliers=4 if ok else 0, H=H,
                    mask=np.full(4, ok), hyp=hyp)
    niters, best, best_k, k = max_iters, 0, -1, 0
    while k < niters:
        idx, H, cnt, _ = hyp.get(k)
        if idx is None:
            if k == 0:
                best_k = -1
            break
        if cnt > max(best, 3):
            best, best_k = cnt, k
            niters = update_num_iters(conf, (n - cnt) / n, 4, niters)
        k += 1
    if best_k < 0:
        return dict(status=2, best_k=-1, iterations=k, n_inliers=0, H=None, mask=np.zeros(n, bool), hyp=hyp)
    H = hyp.get(best_k)[1]
    return dict(status=0, best_k=best_k, iterations=k, n_inliers=best, H=H,
                mask=errors_f32(H, hyp.pa, hyp.pb) <= hyp.thr2, hyp=hyp)


def geometric_optimum(H0, pa, pb, iters=200):
    """fp64 Levenberg-Marquardt on h0..h7 (h33 = 1) of sum |proj(H, a) - b|^2, to convergence."""
    a, b = pa.astype(np.float64), pb.astype(np.float64)
    h = np.asarray(H0, np.float64).reshape(-1)[:8] / np.asarray(H0, np.float64).reshape(-1)[8]

    def resid_jac(h):
        x, y = a[:, 0], a[:, 1]
        inv = 1.0 / (h[6] * x + h[7] * y + 1.0)
        u, v = (h[0] * x + h[1] * y + h[2]) * inv, (h[3] * x + h[4] * y + h[5]) * inv
        z = np.zeros_like(x)
        ju = np.stack([x * inv, y * inv, inv, z, z, z, -u * x * inv, -u * y * inv], 1)
        jv = np.stack([z, z, z, x * inv, y * inv, inv, -v * x * inv, -v * y * inv], 1)
        return np.concatenate([u - b[:, 0], v - b[:, 1]]), np.concatenate([ju, jv])

    lam = 1e-3
    r, J = resid_jac(h)
    e = float(r @ r)
    for _ in range(iters):
        A = J.T @ J
        g = J.T @ r
        d = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
        r1, J1 = resid_jac(h + d)
        e1 = float(r1 @ r1)
        if e1 < e:
            h, r, J, e, lam = h + d, r1, J1, e1, lam * 0.1
        else:
            lam *= 10.0
        if lam > 1e20:
            break
    return np.append(h, 1.0).reshape(3, 3)
