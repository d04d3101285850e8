"""numpy restatement of the tracker's visibility rules (DESIGN.md "Visibility mask in the tracker"; csrc/select.hip
woft_tc_select_vis / woft_tc_flags_vis), on top of the keep rule and Sobol selection of tests/fp64_refs.py.

  gate   : correspondence i survives iff it survives the keep rule and float32(p_i) > float32(thr) (strict: p == thr and NaN
           are dropped); count[1], the draw and the compaction see the gated set; weights untouched.
  weight : keep rule unchanged; the output weight is float32(w_i) * float32(p_i), p_i alone without weights.
No transcendental and no reduction: the kernels are compared bit for bit."""
import numpy as np

import fp64_refs as R

GATE, WEIGHT = "gate", "weight"


def keep_rule_vis(dst, tmask, pwmask, gh, gw, vis, mode, thr, check_dst=True):
    """-> bool (gh*gw,).  vis: (gh*gw,) probabilities on the flow grid (source pixel i = y * gw + x), or None."""
    keep = R.keep_rule(dst, tmask, pwmask, gh, gw, check_dst=check_dst)
    if vis is not None and mode == GATE:
        p = np.asarray(vis, np.float32).reshape(-1)
        with np.errstate(invalid="ignore"):
            keep = keep & (p > np.float32(thr))
    return keep


def select_vis(dst, w, tmask, pwmask, gh, gw, u, cap, vis, mode, thr, check_dst=True):
    """tc_select_vis's outputs: (pa, pb, w_out, count[0], count[1]) for the first min(M, cap) selected correspondences."""
    keep = keep_rule_vis(dst, tmask, pwmask, gh, gw, vis, mode, thr, check_dst=check_dst)
    kept = np.nonzero(keep)[0]
    chosen = kept[R.sobol_ranks(len(kept), u)][:cap]
    d = np.asarray(dst, np.float32).reshape(2, -1)
    pa = d[:, chosen].T
    pb = np.stack([chosen % gw, chosen // gw], 1).astype(np.float32)
    wo = np.ones(len(chosen), np.float32) if w is None else np.asarray(w, np.float32).reshape(-1)[chosen]
    if vis is not None and mode == WEIGHT:
        p = np.asarray(vis, np.float32).reshape(-1)[chosen]
        wo = p.copy() if w is None else (wo * p).astype(np.float32)
    return pa, pb, wo, len(chosen), len(kept)
