"""The planar tracker on multi-delta chained flow: MultiFlowTracker's per-pixel best chains as the correspondences of the
homography fit.  DESIGN.md section 19.

    corr = chain_correspondences(multi.track(frame), mask)      # corr.dst (2, n), corr.w (1, n), corr.ok (1, n), corr.hist (130,)

    trk = WOFTChained(load_config("pytracking/configs/WOFT_chained.py"))
    trk.init(frame0, mask)
    H_cur2init, meta = trk.track(frame1)

One HIP launch (woft_chain_tc, csrc/flow_multi.hip) turns a fold result into target coordinates, the fit weight exp(-cost) -- the
product of the chain's sigmoid(reliability logit) --, the 0 / 1 occlusion gate and the histogram of winning candidates under the
template mask.  Forward only: no autograd graph.  There is no CPU implementation.
"""
import logging
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .multiflow import MultiFlowTracker, _check_constants, _dev32
from .tracker import YAOFTrackerSingleControl

logger = logging.getLogger(__name__)

DEFAULT_DELTAS = (None, 1, 2, 4, 8, 16, 32)


def _mask_u8(mask, h, w):
    """(H, W) uint8 / bool array or tensor, H >= h, W >= w -> (contiguous uint8 device tensor, (H, W)); None -> (None, None)."""
    if mask is None:
        return None, None
    m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask))
    if m.dim() != 2 or m.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"mask: an (H, W) uint8 or bool array is expected, got {tuple(m.shape)} {m.dtype}")
    if m.shape[0] < h or m.shape[1] < w:
        raise ValueError(f"mask: {tuple(m.shape)} is smaller than the flow grid {(h, w)}")
    return m.detach().to("cuda").to(torch.uint8).contiguous(), (int(m.shape[0]), int(m.shape[1]))


def chain_correspondences(result, mask=None, vis_thr=0.5, weights=True):
    """What MultiFlowTracker.track returned -- or a (flow (2, H, W), cost, vis, sel int32) tuple, as chain_fold returns it -- as
    correspondences for a planar fit -> SimpleNamespace(dst (2, n), w (1, n) | None, ok (1, n), hist (130,) int32), n = H * W,
    new tensors.

    dst:  where each template pixel is in the frame, pixel + flow in fp32 (row 0 = x, row 1 = y; the layout ops.tc_select* reads);
          NaN where no chain was valid.
    w:    exp(-cost), 0 where no chain was valid (weights=False: None, nothing is computed).
    ok:   1.0 where a chain was valid and its visibility is not below vis_thr (the fold's rule: vis == vis_thr is visible), else
          0.0 -- a gate at 0.5 for ops.tc_select_vis.
    hist: over the pixels of `mask` (an (H', W') uint8 / bool array at least as large as the flow grid, pixel (x, y) of the grid
          at mask[y, x]; None: every pixel): hist[k] = visible pixels whose best chain is candidate k, hist[128] = pixels
          without a valid chain, hist[129] = valid but occluded pixels.
    Host tensors are copied to the device and the result is handed back on their device.  Computed in fp32."""
    vis_thr, _ = _check_constants(vis_thr, 0.0)
    if isinstance(result, (tuple, list)):
        if len(result) != 4:
            raise ValueError("chain_correspondences: result is a MultiFlowTracker.track() result or (flow, cost, vis, sel)")
        flow, cost, vis, sel = result
    else:
        flow, cost, vis, sel = result.flow, result.cost, result.vis, result.sel
    if not isinstance(flow, torch.Tensor) or flow.dim() != 3 or flow.shape[0] != 2:
        raise ValueError("chain_correspondences: the flow must be a (2, H, W) tensor")
    h, w = flow.shape[1:]
    n = h * w
    if not isinstance(sel, torch.Tensor) or sel.dtype != torch.int32 or sel.numel() != n:
        raise ValueError("chain_correspondences: sel must be an int32 tensor with one entry per pixel")
    tmask, mask_hw = _mask_u8(mask, h, w)
    dst, wts, ok, hist = ops.chain_tc(_dev32(flow, "flow"), _dev32(cost, "cost", n), _dev32(vis, "vis", n),
                                      sel.detach().to("cuda").contiguous(), tmask, vis_thr, want_w=bool(weights), mask_hw=mask_hw)
    dev = flow.device
    return SimpleNamespace(dst=dst.to(dev), w=None if wts is None else wts.to(dev), ok=ok.to(dev), hist=hist.to(dev))


def _set(config, key):
    """Whether a config key is present and truthy (an absent key reads as an empty, falsy Config)."""
    v = getattr(config, key)
    return not isinstance(v, type(config)) and bool(v)


def _get(config, key, default):
    v = getattr(config, key)
    return default if (isinstance(v, type(config)) or v is None) else v


class WOFTChained(YAOFTrackerSingleControl):
    """YAOFTrackerSingleControl whose correspondences are MultiFlowTracker's chains (this project's own, no counterpart in the
    reference): per frame the K flows of `chain_deltas` are folded into the per-pixel most reliable chain template -> frame, one
    woft_chain_tc launch turns it into correspondences, and the parent's solver (either back end) fits the homography to those
    inside the template mask that land in the frame and are not occluded.  There is no pre-warp and no frame t-1 -> t stage: the
    chains are the local motion model.  State, solver back ends and the first-frame announcements are the parent's.

    Config keys, all optional: chain_deltas (default (None, 1, 2, 4, 8, 16, 32)), chain_vis_thr (0.5), chain_unit_cost (1.0),
    chain_iters (None: the flow config's), chain_weights (True; False, or an unweighted estimator preset: exp(-cost) is not
    computed and the fit is unweighted), chain_share_features (False; True: every frame is encoded once and its flows run from the
    record -- MultiFlowTracker(share_features=True), bit-identical, 66.4 MB more per stored 1080p frame).  raft_type 'orig' chains on unit costs (w = exp(-chain_unit_cost * chain length)),
    'weighted' on the reliability logit, 'weighted_masked' also on the visibility logit -- without a `visibility_mode`: the fold
    consumes the mask.  `pw_mask`, `no_prewarp_after_N`, `no_local_H` and `do_not_mask_TCs_by_prewarped` are not used.

    A frame is lost when the fit is rejected (its H is still returned, the parent's `no_local_H` behaviour) or when fewer than
    4 correspondences survive or H is not finite (the previous pose is returned).  meta: lost, N_lost, global_H_success,
    H_global_cur2init (None when there was no usable fit), n_kept, chain_hist (int64 numpy, visible mask pixels per delta),
    chain_invalid, chain_occluded (mask pixels without a valid chain / with an occluded one)."""
    MASK_NEEDS_VISIBILITY_MODE = False            # ('weighted_masked' without a visibility_mode: the fold reads the mask)

    REFUSED = (
        ("visibility_mode", "the fold consumes the visibility mask of a 'weighted_masked' flow config itself (chain_vis_thr)"),
        ("fb_check", "the solver's one visibility slot carries the chains' occlusion gate"),
        ("warm_start_local", "there is no frame t-1 -> t stage to warm-start"),
        ("downscale_inputs", "the stored frames and results of the chains are kept at the input's size"),
        ("search_window_margin", "the chains read every pixel of every flow; the search-window tracker is WOFTWindow"),
        ("post_hoc_weights_postprocessing_fn", "the fit weight is exp(-chain cost), not a weight map to post-process"),
    )

    def __init__(self, config):
        for key, why in self.REFUSED:
            if _set(config, key):
                raise NotImplementedError(f"{key} is not provided by the chained tracker: {why}")
        if _set(config.flow_config, "weights_postprocessing_fn"):
            raise NotImplementedError("the chained tracker's chain cost is defined on the raw reliability logit; a flow config with "
                                      "a weights_postprocessing_fn is not supported")
        self.chain_deltas = _get(config, "chain_deltas", DEFAULT_DELTAS)
        self.chain_vis_thr = _get(config, "chain_vis_thr", 0.5)
        self.chain_unit_cost = _get(config, "chain_unit_cost", 1.0)
        self.chain_iters = _get(config, "chain_iters", None)
        self.chain_weights = bool(_get(config, "chain_weights", True))
        self.chain_share_features = bool(_get(config, "chain_share_features", False))
        super().__init__(config)
        if not hasattr(self.flower, "pin_source"):
            raise NotImplementedError("the chained tracker needs this project's flow provider (pin_source, compute_flow(mode='flow', "
                                      f"borrow=True)); {type(self.flower).__name__} has no pin_source")
        self.multi = self._new_multi()            # (validates the chain keys)
        self.chain_deltas = self.multi.deltas
        self.solver_decision += (f"; chained deltas {self.chain_deltas}; chain_share_features "
                                 f"{'on: every frame encoded once' if self.chain_share_features else 'off'}; pw_mask, no_prewarp_after_N, no_local_H and "
                                 "do_not_mask_TCs_by_prewarped are not used")
        if self._fused is not None and not self.chain_weights:
            self._fused = dict(self._fused, weighted=False)
        # the solver's visibility slot carries the chains' 0 / 1 occlusion gate, the way fb_check hands its verdict
        self._vis_mode, self._vis_thr = "gate", 0.5
        self._tc = {}                             # per grid size: the outputs of chain_tc, reused
        self._grid = {}                           # per grid size: the (2, n) int64 source grid (callable back end only)

    def _new_multi(self):
        return MultiFlowTracker(self.flower, deltas=self.chain_deltas, vis_thr=self.chain_vis_thr, unit_cost=self.chain_unit_cost,
                                iters=self.chain_iters, share_features=self.chain_share_features)

    def _device_solver_reads(self, raft_type):
        return True                               # (weights and gate come from chain_tc, whatever the network provides)

    def _wants_weights(self):
        return self.chain_weights and (self._fused is None or self._fused.get("weighted", True))

    def init(self, img, mask, img_identifier=None):
        super().init(img, mask, img_identifier)                      # (single-contour check, mask tensors, state: the parent's)
        self.multi = self._new_multi()
        self.multi.init(img)
        # the chains read every pixel of every flow: no weight region, no flow region, no deferred weights
        if hasattr(self.flower, "pin_weight_region"):
            self.flower.pin_weight_region(None)
        if hasattr(self.flower, "pin_flow_region"):
            self.flower.pin_flow_region(None)
        self._sparse_weights = False

    def set_fast_meta(self, meta):
        raise NotImplementedError("Fastforward is not provided by the chained tracker: a replayed frame would leave a hole in the "
                                  "ring of stored frames the chains reach back to")

    def _source_grid(self, gh, gw):
        if (gh, gw) not in self._grid:
            i = torch.arange(gh * gw, device=self.device)
            self._grid = {(gh, gw): torch.stack([i % gw, torch.div(i, gw, rounding_mode="floor")])}
        return self._grid[(gh, gw)]

    def track(self, input_img, debug=False, img_identifier=None):
        meta = SimpleNamespace()
        self._n_tracked += 1
        out = self.multi.track(input_img)                            # (uploads the frame: the ring keeps a copy of its own)
        Hh, Ww = int(input_img.shape[0]), int(input_img.shape[1])
        gh, gw = int(out.flow.shape[1]), int(out.flow.shape[2])
        dst, w, ok, hist = self._tc[(gh, gw)] = ops.chain_tc(out.flow, out.cost, out.vis, out.sel, self._template_mask_u8,
                                                             self.chain_vis_thr, want_w=self._wants_weights(), mask_hw=(Hh, Ww),
                                                             out=self._tc.get((gh, gw)))
        src_xy = None if self._fused is not None else self._source_grid(gh, gw)
        self.n_kept = None
        try:
            fit = self._solve(src_xy, dst, w, (gh, gw), (Hh, Ww), self._template_mask_u8, None, bounds=True, judge=True, vis=ok)
        except AssertionError:                                       # (too few correspondences for the estimator)
            fit = None
        usable = (fit is not None and not (self.n_kept is not None and self.n_kept < 4) and bool(np.all(np.isfinite(fit.H))))
        meta.n_kept = self.n_kept
        meta.H_global_cur2init = fit.H.copy() if usable else None
        success = bool(usable and fit.success)
        logger.debug(f"global_H_success: {success}")
        if success:
            self.lost, self.N_lost = False, 0
        else:
            self.lost, self.N_lost = True, self.N_lost + 1
        # the fit maps current -> template; a rejected fit is still returned, no usable fit keeps the previous pose
        H_cur2init = fit.H if usable else self.prev_H2init
        self.prev_img, self.prev_img_identifier = input_img, img_identifier
        self._set_pose(H_cur2init.copy(), good=not self.lost)
        meta.lost, meta.N_lost, meta.global_H_success = self.lost, self.N_lost, success
        counts = hist.cpu().numpy().astype(np.int64)
        meta.chain_hist = counts[:len(self.chain_deltas)].copy()
        meta.chain_invalid, meta.chain_occluded = int(counts[ops.CHAIN_HIST - 2]), int(counts[ops.CHAIN_HIST - 1])
        if not self._announced:
            self._announced = True
            meta.precision = getattr(self.flower, "precision", None)
            meta.precision_source = getattr(self.flower, "precision_source", None)
            meta.solver_decision = self.solver_decision
        return H_cur2init.copy(), meta
