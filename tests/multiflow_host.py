"""numpy restatement of csrc/flow_multi.hip (test infrastructure).

  * fold: one candidate folded into a running best, in `dtype` arithmetic from fp32 inputs, in the kernel's operation order; q =
    pixel + prev flow is formed in fp32 in either dtype, so that validity is decided on the very numbers the kernel decides it on.
  * fold_all: the loop over candidates.  In float64 it also returns the two margins that say how far the case is from a decision a
    rounding error could turn: (a) the smallest |cost - best_cost| over all comparisons that were decided by cost, (b) the smallest
    |vis - vis_thr| over valid candidates.
  * make_case: the fixed recipe of the generated test cases.

No index is ever formed from an unclamped value: the tap indices come from floats forced into the plane first, as in the kernel.
"""
import numpy as np

F32 = np.float32


def _clamp32(v, hi):
    """v forced into [0, hi] the way the kernel does it: NaN -> 0, +inf -> hi, -inf -> 0 (two ordered compares)."""
    lo = np.where(v >= 0, v, F32(0)).astype(F32)
    return np.where(lo <= hi, lo, F32(hi)).astype(F32)


def taps(pflow):
    """(2, H, W) fp32 prev flow (None: the template itself) -> dict(valid, i00, i01, i10, i11 (flat indices, always in the plane),
    ax, ay fp32): where each pixel's q lands."""
    _, h, w = pflow.shape
    ys, xs = np.mgrid[:h, :w]
    with np.errstate(all="ignore"):
        qx = (xs.astype(F32) + pflow[0]).astype(F32)
        qy = (ys.astype(F32) + pflow[1]).astype(F32)
        valid = (qx >= 0) & (qx <= F32(w - 1)) & (qy >= 0) & (qy <= F32(h - 1))
        x0f, y0f = _clamp32(np.floor(qx), F32(w - 1)), _clamp32(np.floor(qy), F32(h - 1))
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        ax, ay = (qx - x0f).astype(F32), (qy - y0f).astype(F32)
    return dict(valid=valid, i00=y0 * w + x0, i01=y0 * w + x1, i10=y1 * w + x0, i11=y1 * w + x1, ax=ax, ay=ay)


def sample(plane, t, dtype):
    """(1-ay)*((1-ax)*d00 + ax*d01) + ay*((1-ax)*d10 + ax*d11) in `dtype`, every product and sum rounded on its own."""
    f = np.asarray(plane, F32).reshape(-1).astype(dtype)
    ax, ay = t["ax"].astype(dtype), t["ay"].astype(dtype)
    bx, by = dtype(1) - ax, dtype(1) - ay
    with np.errstate(all="ignore"):
        return by * (bx * f[t["i00"]] + ax * f[t["i01"]]) + ay * (bx * f[t["i10"]] + ax * f[t["i11"]])


def softplus_neg(l):
    """softplus(-l) as the kernel takes it: l < 0: -l + log1p(exp(l)), else log1p(exp(-l))."""
    with np.errstate(all="ignore"):
        return np.where(l < 0, -l + np.log1p(np.exp(np.where(l < 0, l, 0))), np.log1p(np.exp(-np.where(l < 0, 0, l))))


def candidate(prev, step, unit_cost, dtype):
    """-> (valid (H, W) bool, flow (2, H, W), cost, vis (H, W)) of one candidate, in `dtype`.
    prev: None or (flow (2, H, W), cost (H, W), vis (H, W)); step: (flow, wlogit | None, mlogit | None); all fp32."""
    sflow = np.asarray(step[0], F32)
    _, h, w = sflow.shape
    if prev is None:
        pflow, pcost, pvis = np.zeros((2, h, w), F32), np.zeros((h, w), F32), np.ones((h, w), F32)
    else:
        pflow, pcost, pvis = (np.asarray(p, F32) for p in prev)
    t = taps(pflow)
    ok = t["valid"].copy()
    with np.errstate(all="ignore"):
        flow = pflow.astype(dtype) + np.stack([sample(sflow[0], t, dtype), sample(sflow[1], t, dtype)])
        cost = pcost.reshape(h, w).astype(dtype) + dtype(F32(unit_cost))
        vis = pvis.reshape(h, w).astype(dtype)
        if step[1] is not None:
            l = sample(step[1], t, dtype)
            ok &= np.isfinite(l)
            cost = pcost.reshape(h, w).astype(dtype) + softplus_neg(l).astype(dtype)
        if step[2] is not None:
            m = sample(step[2], t, dtype)
            ok &= np.isfinite(m)
            vis = pvis.reshape(h, w).astype(dtype) * (dtype(1) / (dtype(1) + np.exp(-m))).astype(dtype)
    ok &= np.isfinite(flow[0]) & np.isfinite(flow[1]) & np.isfinite(cost) & np.isfinite(vis)
    return ok, flow.astype(dtype), cost.astype(dtype), vis.astype(dtype)


def empty(h, w, dtype):
    return dict(flow=np.full((2, h, w), np.nan, dtype), cost=np.full((h, w), np.inf, dtype), vis=np.zeros((h, w), dtype),
                sel=np.full((h, w), -1, np.int32))


def fold(best, prev, step, k, vis_thr=0.5, unit_cost=1.0, dtype=np.float64, margins=None):
    """One fold -> the new best (a dict flow, cost, vis, sel; `best` = None starts the fold and is otherwise left alone).
    margins: a dict whose 'cost' and 'vis' entries are lowered to this fold's smallest margins."""
    ok, flow, cost, vis = candidate(prev, step, unit_cost, dtype)
    h, w = ok.shape
    out = empty(h, w, dtype) if best is None else {n: v.copy() for n, v in best.items()}
    thr = dtype(F32(vis_thr))
    with np.errstate(all="ignore"):
        occ, bocc, filled = vis < thr, out["vis"] < thr, out["sel"] >= 0
        by_cost = ok & filled & (occ == bocc)
        replace = ok & (~filled | (bocc & ~occ) | (by_cost & (cost < out["cost"])))
        if margins is not None:
            if by_cost.any():
                margins["cost"] = min(margins["cost"], float(np.abs(cost - out["cost"])[by_cost].min()))
            if ok.any():
                margins["vis"] = min(margins["vis"], float(np.abs(vis - thr)[ok].min()))
    out["flow"][:, replace], out["cost"][replace], out["vis"][replace] = flow[:, replace], cost[replace], vis[replace]
    out["sel"][replace] = k
    return out


def fold_all(cands, vis_thr=0.5, unit_cost=1.0, dtype=np.float64, order=None):
    """The fold loop over cands = [(prev, step)], candidate k = its position in the list, folded in `order` (default 0, 1, ...)
    -> (best, margins): margins = dict(cost=(a), vis=(b)), +inf where no such comparison happened."""
    margins = dict(cost=np.inf, vis=np.inf)
    best = None
    for k in (range(len(cands)) if order is None else order):
        best = fold(best, cands[k][0], cands[k][1], k, vis_thr, unit_cost, dtype, margins)
    return best, margins


CASES = ((5, 7, 1), (9, 70, 3), (37, 131, 7))


def _smooth(h, w, amp, rs):
    """A sinusoidal (h, w) field of amplitude `amp` with a seeded phase and a period of the order of the frame."""
    ys, xs = np.mgrid[:h, :w].astype(np.float64)
    p = rs.uniform(0, 2 * np.pi, 2)
    fx, fy = rs.uniform(0.7, 1.6, 2) * 2 * np.pi / np.array([max(w, 8), max(h, 8)])
    return amp * np.sin(fx * xs + p[0]) * np.cos(fy * ys + p[1])


def make_case(h, w, K, seed=0):
    """The generated cases (fixed recipe) -> [(prev, step)] * K, fp32: smooth sinusoidal flows of amplitude 3 px (prev) and 2 px
    (step); prev_cost = 0.5 * rank_k(pixel) + U(0, 0.05) with a random per-pixel permutation of the ranks 0..K-1; prev_vis from
    the bands [0.05, 0.3] (probability 0.3) and [0.7, 1]; both logit maps 3 + a smooth term of amplitude 0.3.
    Margins by construction: step costs lie in softplus(-3.3) .. softplus(-2.7) = 0.036 .. 0.065, so two candidates' costs differ by
    at least 0.5 - 0.05 - 0.03 = 0.42; vis = prev_vis * sigmoid(2.7 .. 3.3) lies in [0.047, 0.29] or [0.656, 0.964], at least
    0.15 from the threshold 0.5."""
    rs = np.random.RandomState(7000 + 131 * h + 17 * w + K + seed)
    ranks = np.argsort(rs.uniform(size=(K, h, w)), axis=0)
    out = []
    for k in range(K):
        pflow = np.stack([_smooth(h, w, 3.0, rs), _smooth(h, w, 3.0, rs)]).astype(F32)
        sflow = np.stack([_smooth(h, w, 2.0, rs), _smooth(h, w, 2.0, rs)]).astype(F32)
        pcost = (0.5 * ranks[k] + rs.uniform(0, 0.05, (h, w))).astype(F32)
        low = rs.uniform(size=(h, w)) < 0.3
        pvis = np.where(low, rs.uniform(0.05, 0.3, (h, w)), rs.uniform(0.7, 1.0, (h, w))).astype(F32)
        wl, ml = (3.0 + _smooth(h, w, 0.3, rs)).astype(F32), (3.0 + _smooth(h, w, 0.3, rs)).astype(F32)
        out.append(((pflow, pcost, pvis), (sflow, wl, ml)))
    return out
