"""numpy restatement of woft_chain_tc (csrc/flow_multi.hip; test infrastructure).

  * chain_tc: a fold result -> dst, w, ok, hist in `dtype` arithmetic from fp32 inputs, in the kernel's operation order.  The
    two compares that decide `ok` and `hist` (finiteness, vis < vis_thr) are exact in either dtype; dst = (float)pixel + flow is
    one add, exact in float64 and therefore, rounded to fp32, the fp32 sum; only w = exp(-cost) differs between the dtypes.
  * make_case: the fixed recipe of the generated cases, with the planted pixels the tests look at.

No index is formed from a field's value except `sel`, range-checked first, as in the kernel.
"""
import numpy as np

F32 = np.float32
HIST = 130
INVALID, OCCLUDED = 128, 129

# (h, w, K, mask_hw): under one wave; a row tail across the 64-wide tile; several blocks; rows beyond one grid pass (65535 * 4);
# the 'crop' geometry -- a flow grid inside a larger frame-sized mask
CASES = ((5, 7, 1, None), (9, 70, 3, None), (37, 131, 7, None), (4 * 65535 + 5, 1, 2, None), (24, 40, 3, (29, 45)))


def chain_tc(flow, cost, vis, sel, tmask=None, vis_thr=0.5, dtype=np.float64):
    """-> dict(dst (2, n) `dtype`, w (1, n) `dtype`, ok (1, n) float32, hist (130,) int32, valid (h, w) bool).
    flow (2, h, w), cost, vis (h, w) fp32, sel (h, w) int32; tmask: None or a (mh, mw) array, mh >= h, mw >= w."""
    flow = np.asarray(flow, F32)
    _, h, w = flow.shape
    cost, vis = np.asarray(cost, F32).reshape(h, w), np.asarray(vis, F32).reshape(h, w)
    sel = np.asarray(sel, np.int32).reshape(h, w)
    ys, xs = np.mgrid[:h, :w]
    valid = (sel >= 0) & (sel <= 127) & np.isfinite(flow[0]) & np.isfinite(flow[1]) & np.isfinite(cost) & np.isfinite(vis)
    with np.errstate(all="ignore"):
        dst = np.stack([xs.astype(F32).astype(dtype) + flow[0].astype(dtype), ys.astype(F32).astype(dtype) + flow[1].astype(dtype)])
        dst[:, ~valid] = np.nan
        wts = np.where(valid, np.exp(-cost.astype(dtype)), dtype(0)).astype(dtype)
        ok = valid & ~(vis.astype(dtype) < dtype(F32(vis_thr)))
    m = np.ones((h, w), bool) if tmask is None else (np.asarray(tmask)[:h, :w] != 0)
    hist = np.zeros(HIST, np.int64)
    hist[:128] = np.bincount(sel[ok & m], minlength=128)
    hist[INVALID], hist[OCCLUDED] = (~valid & m).sum(), (valid & ~ok & m).sum()
    return dict(dst=dst.reshape(2, -1), w=wts.reshape(1, -1), ok=ok.astype(F32).reshape(1, -1), hist=hist.astype(np.int32), valid=valid)


PLANTS = ([("sel", np.int32(-1)), ("sel", np.int32(127)), ("sel", np.int32(128)), ("sel", np.int32(2 ** 31 - 1)), ("vis", "thr")]
          + [(name, v) for name in ("flow_x", "flow_y", "cost", "vis") for v in (np.nan, np.inf, -np.inf)])


def make_case(h, w, K, seed=0, mask_hw=None, vis_thr=0.5, plant=True):
    """-> dict(flow (2, h, w), cost, vis (h, w) fp32, sel (h, w) int32, mask (mask_hw or (h, w)) uint8, vis_thr,
    planted = [(flat pixel, field, value)]).  Smooth flows of a few pixels, cost in [0, 3], vis from the bands [0.05, 0.3]
    (probability 0.3) and [0.7, 1] -- at least 0.2 from the thresholds 0.5 and 0.3 the tests use, not that the exact compare needs
    it --, sel uniform in 0..K-1, a mask with about 70 % of its pixels set.  plant: at len(PLANTS) pixels spread evenly over the
    plane, first and last pixel included, one field each is replaced: sel = -1, 127 (valid: the last counter), 128 and 2^31 - 1
    (invalid: never written by the fold), vis == vis_thr exactly (not occluded), and NaN / +inf / -inf in each of flow_x, flow_y,
    cost, vis.  plant=False: the same fields without them."""
    rs = np.random.RandomState(9000 + 131 * h + 17 * w + K + seed)
    ys, xs = np.mgrid[:h, :w].astype(np.float64)
    wave = lambda amp: amp * np.sin(xs * rs.uniform(0.05, 0.2) + ys * rs.uniform(0.05, 0.2) + rs.uniform(0, 6))
    flow = np.stack([wave(3.0), wave(3.0)]).astype(F32)
    cost = rs.uniform(0, 3, (h, w)).astype(F32)
    vis = np.where(rs.uniform(size=(h, w)) < 0.3, rs.uniform(0.05, 0.3, (h, w)), rs.uniform(0.7, 1.0, (h, w))).astype(F32)
    sel = rs.randint(0, K, (h, w)).astype(np.int32)
    mask = (rs.uniform(size=mask_hw or (h, w)) < 0.7).astype(np.uint8) * 255
    planted = []
    if plant:
        n = h * w
        at = np.linspace(0, n - 1, len(PLANTS)).astype(np.int64)
        assert len(set(at.tolist())) == len(PLANTS), "the plane is too small for the planted pixels"
        fields = dict(flow_x=flow[0].reshape(-1), flow_y=flow[1].reshape(-1), cost=cost.reshape(-1), vis=vis.reshape(-1),
                      sel=sel.reshape(-1))                          # (views: the assignments below write the fields)
        for i, (name, v) in zip(at.tolist(), PLANTS):
            v = F32(vis_thr) if isinstance(v, str) else v
            fields[name][i] = v
            if name == "sel" and v == 127:
                fields["vis"][i] = F32(0.9)                          # (visible: it is counted in hist[127])
            planted.append((i, name, v))
            mask[i // w, i % w] = 255                                # (every planted pixel counts in the histogram)
    return dict(flow=flow, cost=cost, vis=vis, sel=sel, mask=mask, vis_thr=vis_thr, planted=planted)
