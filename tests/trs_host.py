"""Host restatement of the RANSAC similarity estimator of woft_amd/csrc/trs.hip (a helper of the TRS tests, not a conftest): the
SplitMix64 index stream of tests/ransac_host.py, the closed-form fp64 two-point model, cv2's fp32 error formula and cv2's
SEQUENTIAL selection loop with two model points (RANSACUpdateNumIters after every new best), written as plainly as possible; every
fp64 / fp32 operation in the order the kernel performs it, so that the per-hypothesis inlier counts agree exactly.
`refit` is the fp64 closed-form least-squares similarity over an inlier set."""
import math

import numpy as np

from ransac_host import DBL_MIN, M64, draw_index, splitmix64


def draw_pair(n, key, k):
    """-> the 2 distinct indices of hypothesis k (cv2 checks nothing else about a two-point sample)."""
    c = 0
    i0 = draw_index(key, k, c, n)
    c += 1
    while True:
        i1 = draw_index(key, k, c, n)
        c += 1
        if i1 != i0:
            return [i0, i1]


def model2(a, b):
    """Two-point similarity a -> b: q = (B1 - B0) conj(A1 - A0) / |A1 - A0|^2, t = B0 - q A0 -> [Re q, Im q, Re t, Im t]
    (Python floats), or None when degenerate."""
    a0x, a0y, a1x, a1y = (float(v) for v in a.reshape(-1))
    b0x, b0y, b1x, b1y = (float(v) for v in b.reshape(-1))
    dax, day, dbx, dby = a1x - a0x, a1y - a0y, b1x - b0x, b1y - b0y
    den = dax * dax + day * day
    if den == 0.0:
        return None
    qr, qi = (dbx * dax + dby * day) / den, (dby * dax - dbx * day) / den
    m = [qr, qi, b0x - (qr * a0x - qi * a0y), b0y - (qi * a0x + qr * a0y)]
    return m if all(math.isfinite(v) for v in m) else None


def to_H(m):
    """[Re q, Im q, Re t, Im t] -> (3, 3) float64."""
    return np.array([[m[0], -m[1], m[2]], [m[1], m[0], m[3]], [0.0, 0.0, 1.0]])


def errors_f32(m, pa, pb):
    """cv2's fp32 error of every point, the model cast to fp32 first."""
    qr, qi, tx, ty = (np.float32(v) for v in m)
    x, y, X, Y = pa[:, 0], pa[:, 1], pb[:, 0], pb[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        dx = qr * x + (-qi) * y + tx - X
        dy = qi * x + qr * y + ty - Y
        return dx * dx + dy * dy


def errors_f64(m, pa, pb):
    a, b = pa.astype(np.float64), pb.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = m[0] * a[:, 0] - m[1] * a[:, 1] + m[2] - b[:, 0]
        dy = m[1] * a[:, 0] + m[0] * a[:, 1] + m[3] - b[:, 1]
        return dx * dx + dy * dy


def update_num_iters(p, ep, max_iters):
    """RANSACUpdateNumIters as OpenCV publishes it, for two model points: 1 - (1 - ep)^2 in the denominator."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    t = 1.0 - ep
    denom = 1.0 - t * t
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else int(np.rint(num / denom))


class Hypotheses:
    """Hypothesis k of a fit: its sample, model, fp32 inlier count (0 degenerate) and the number of points whose fp64 error lies
    within 1e-4 thr^2 of thr^2 (where an fp32 decision may legitimately differ)."""

    def __init__(self, pa, pb, thr, seed):
        self.pa, self.pb = np.ascontiguousarray(pa, np.float32), np.ascontiguousarray(pb, np.float32)
        self.thr2 = np.float32(float(thr) * float(thr))
        self.key = splitmix64(int(seed) & M64)
        self._cache = {}

    def get(self, k):
        if k not in self._cache:
            idx = draw_pair(self.pa.shape[0], self.key, k)
            m = model2(self.pa[idx], self.pb[idx])
            if m is None:
                cnt, near = 0, 0
            else:
                cnt = int((errors_f32(m, self.pa, self.pb) <= self.thr2).sum())
                near = int((np.abs(errors_f64(m, self.pa, self.pb) - float(self.thr2)) <= 1e-4 * float(self.thr2)).sum())
            self._cache[k] = (idx, m, cnt, near)
        return self._cache[k]


def trs_host(pa, pb, max_iters=10000, thr=3.0, conf=0.999, seed=0):
    """cv2's sequential loop -> dict(status, best_k, iterations, n_inliers, m (best two-point model), mask, hyp (Hypotheses))."""
    n = pa.shape[0]
    assert n >= 2
    hyp = Hypotheses(pa, pb, thr, seed)
    if n == 2:
        m = model2(hyp.pa, hyp.pb)
        ok = m is not None
        return dict(status=0 if ok else 2, best_k=0 if ok else -1, iterations=0, n_inliers=2 if ok else 0, m=m,
                    mask=np.full(2, ok), hyp=hyp)
    niters, best, best_k, k = max_iters, 0, -1, 0
    while k < niters:
        cnt = hyp.get(k)[2]
        if cnt > max(best, 1):
            best, best_k = cnt, k
            niters = update_num_iters(conf, (n - cnt) / n, niters)
        k += 1
    if best_k < 0:
        return dict(status=2, best_k=-1, iterations=k, n_inliers=0, m=None, mask=np.zeros(n, bool), hyp=hyp)
    m = hyp.get(best_k)[1]
    return dict(status=0, best_k=best_k, iterations=k, n_inliers=best, m=m, mask=errors_f32(m, hyp.pa, hyp.pb) <= hyp.thr2,
                hyp=hyp)


def refit(pa, pb):
    """fp64 closed-form least-squares similarity pa -> pb: centroids abar, bbar, q = sum (b - bbar) conj(a - abar) /
    sum |a - abar|^2, t = bbar - q abar -> [Re q, Im q, Re t, Im t], or None when the a all coincide."""
    a = pa.astype(np.float64)[:, 0] + 1j * pa.astype(np.float64)[:, 1]
    b = pb.astype(np.float64)[:, 0] + 1j * pb.astype(np.float64)[:, 1]
    ca, cb = a.mean(), b.mean()
    den = float((np.abs(a - ca) ** 2).sum())
    if not den > 0.0:
        return None
    q = ((b - cb) * np.conj(a - ca)).sum() / den
    t = cb - q * ca
    return [float(q.real), float(q.imag), float(t.real), float(t.imag)]


def fit_host(pa, pb, max_iters=10000, thr=3.0, conf=0.999, seed=0, refine=True):
    """The whole estimator -> trs_host's dict plus H (3, 3) float64 (all NaN without a model)."""
    r = trs_host(pa, pb, max_iters, thr, conf, seed)
    if r["status"] != 0:
        r["H"] = np.full((3, 3), np.nan)
        return r
    m = r["m"]
    if refine and pa.shape[0] > 2 and r["n_inliers"] > 2:
        m = refit(r["hyp"].pa[r["mask"]], r["hyp"].pb[r["mask"]]) or m
    r["H"] = to_H(m)
    return r
