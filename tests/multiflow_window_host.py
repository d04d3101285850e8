"""numpy restatement of the rectangle form of the fold (woft_flow_chain_fold_window, csrc/flow_multi.hip), built
on multiflow_host: the sampler, softplus, the empty pixel and the recipe of the generated cases are that module's.

  * candidate: one candidate on a template rectangle and a step rectangle, in `dtype` arithmetic from fp32 inputs, in the kernel's
    operation order; q = P + prev flow and u = q - (step origin) are formed in fp32 in either dtype, so that validity is decided on
    the very numbers the kernel decides it on.  post_H: the closing homography, always in float64 with one rounding to `dtype`.
  * fold, fold_all: multiflow_host's decision rule on such candidates; fold_all takes a step rectangle per candidate.
  * crop / crop_case: planes of a full-frame case cut to rectangles.

A rectangle is (y0, x0, rows, cols).  No index is formed from an unclamped value.
"""
import numpy as np

import multiflow_host as MH

F32 = np.float32


def crop(a, rect):
    y0, x0, rows, cols = rect
    return np.ascontiguousarray(np.asarray(a)[..., y0:y0 + rows, x0:x0 + cols])


def crop_case(prev, step, trect, srect):
    """A full-frame (prev, step) pair of make_case -> the pair on the two rectangles."""
    return (None if prev is None else tuple(crop(p, trect) for p in prev),
            tuple(None if s is None else crop(s, srect) for s in step))


def taps(ux, uy, sh, sw):
    """fp32 window coordinates -> multiflow_host.taps' dict for an sh x sw plane."""
    with np.errstate(all="ignore"):
        valid = (ux >= 0) & (ux <= F32(sw - 1)) & (uy >= 0) & (uy <= F32(sh - 1))
        x0f, y0f = MH._clamp32(np.floor(ux), F32(sw - 1)), MH._clamp32(np.floor(uy), F32(sh - 1))
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
        ax, ay = (ux - x0f).astype(F32), (uy - y0f).astype(F32)
    return dict(valid=valid, i00=y0 * sw + x0, i01=y0 * sw + x1, i10=y1 * sw + x0, i11=y1 * sw + x1, ax=ax, ay=ay)


def landing(prev_flow, trect, srect):
    """-> (P (2, th, tw) fp32 template pixels, u (2, th, tw) fp32 = P + prev flow - step origin)."""
    ty0, tx0, th, tw = trect
    ys, xs = np.mgrid[ty0:ty0 + th, tx0:tx0 + tw]
    P = np.stack([xs, ys]).astype(F32)
    with np.errstate(all="ignore"):
        q = P if prev_flow is None else (P + np.asarray(prev_flow, F32)).astype(F32)
        u = np.stack([(q[0] - F32(srect[1])).astype(F32), (q[1] - F32(srect[0])).astype(F32)])
    return P, u


def candidate(prev, step, trect, srect, unit_cost, dtype, post_H=None):
    """-> (valid (th, tw) bool, flow (2, th, tw), cost, vis (th, tw)) of one candidate, in `dtype`.
    prev: None or (flow (2, th, tw), cost, vis) on trect; step: (flow (2, sh, sw), wlogit | None, mlogit | None) on srect."""
    _, _, th, tw = trect
    _, _, sh, sw = srect
    sflow = np.asarray(step[0], F32)
    assert sflow.shape == (2, sh, sw)
    if prev is None:
        pflow, pcost, pvis = np.zeros((2, th, tw), F32), np.zeros((th, tw), F32), np.ones((th, tw), F32)
    else:
        pflow, pcost, pvis = (np.asarray(p, F32) for p in prev)
    P, u = landing(None if prev is None else pflow, trect, srect)
    t = taps(u[0], u[1], sh, sw)
    ok = t["valid"].copy()
    with np.errstate(all="ignore"):
        flow = pflow.astype(dtype) + np.stack([MH.sample(sflow[0], t, dtype), MH.sample(sflow[1], t, dtype)])
        cost = pcost.reshape(th, tw).astype(dtype) + dtype(F32(unit_cost))
        vis = pvis.reshape(th, tw).astype(dtype)
        if step[1] is not None:
            l = MH.sample(step[1], t, dtype)
            ok &= np.isfinite(l)
            cost = pcost.reshape(th, tw).astype(dtype) + MH.softplus_neg(l).astype(dtype)
        if len(step) > 2 and step[2] is not None:
            m = MH.sample(step[2], t, dtype)
            ok &= np.isfinite(m)
            vis = pvis.reshape(th, tw).astype(dtype) * (dtype(1) / (dtype(1) + np.exp(-m))).astype(dtype)
        if post_H is not None:
            Hm = np.asarray(post_H, np.float64)
            P64 = P.astype(np.float64)
            r = P64 + flow.astype(np.float64)
            den = Hm[2, 0] * r[0] + Hm[2, 1] * r[1] + Hm[2, 2]
            mx = (Hm[0, 0] * r[0] + Hm[0, 1] * r[1] + Hm[0, 2]) / den
            my = (Hm[1, 0] * r[0] + Hm[1, 1] * r[1] + Hm[1, 2]) / den
            ok &= (den > 0) & np.isfinite(mx) & np.isfinite(my)
            flow = np.stack([mx - P64[0], my - P64[1]]).astype(dtype)
    ok &= np.isfinite(flow[0]) & np.isfinite(flow[1]) & np.isfinite(cost) & np.isfinite(vis)
    return ok, flow.astype(dtype), cost.astype(dtype), vis.astype(dtype)


def post_den(prev, step, trect, srect, post_H):
    """The float64 denominators of post_H at every template pixel's landing (NaN where the tap is invalid)."""
    ok, flow, _, _ = candidate(prev, step, trect, srect, 1.0, np.float64)
    P, _ = landing(None, trect, srect)
    r = P.astype(np.float64) + flow
    Hm = np.asarray(post_H, np.float64)
    return np.where(ok, Hm[2, 0] * r[0] + Hm[2, 1] * r[1] + Hm[2, 2], np.nan)


def fold(best, prev, step, k, trect, srect, vis_thr=0.5, unit_cost=1.0, dtype=np.float64, margins=None, post_H=None):
    """multiflow_host.fold's decision rule on a rectangle candidate."""
    ok, flow, cost, vis = candidate(prev, step, trect, srect, unit_cost, dtype, post_H)
    th, tw = ok.shape
    out = MH.empty(th, tw, dtype) if best is None else {n: v.copy() for n, v in best.items()}
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


def fold_all(cands, trect, srects, vis_thr=0.5, unit_cost=1.0, dtype=np.float64, order=None):
    """cands = [(prev on trect, step on srects[k])], folded in `order` -> (best, margins), as multiflow_host.fold_all."""
    margins = dict(cost=np.inf, vis=np.inf)
    best = None
    for k in (range(len(cands)) if order is None else order):
        best = fold(best, cands[k][0], cands[k][1], k, trect, srects[k], vis_thr, unit_cost, dtype, margins)
    return best, margins


# the rectangle pairs of the generated cases: (make_case arguments, template rect, step rect); the share of template-rect pixels
# whose q lies in the step rect is 0.484, 0.405 and 0.593 (asserted to lie in [0.25, 0.75] where they are used)
RECT_CASES = (((37, 131, 7), (4, 6, 24, 40), (8, 10, 16, 32)),
              ((9, 70, 3), (1, 3, 7, 50), (2, 8, 6, 40)),
              ((64, 96, 3), (8, 16, 40, 64), (12, 22, 32, 48)))
