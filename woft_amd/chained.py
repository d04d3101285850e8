"""The planar tracker on multi-delta chained flow: MultiFlowTracker's per-pixel best chains as the correspondences of the
homography fit.  DESIGN.md section 19.

    corr = chain_correspondences(multi.track(frame), mask)      # corr.dst (2, n), corr.w (1, n), corr.ok (1, n), corr.hist (130,)

    trk = WOFTChained(load_config("pytracking/configs/WOFT_chained.py"))
    trk.init(frame0, mask)
    H_cur2init, meta = trk.track(frame1)

One HIP launch (woft_chain_tc, csrc/flow_multi.hip) turns a fold result into target coordinates, the fit weight exp(-cost) -- the
product of the chain's sigmoid(reliability logit) --, the 0 / 1 occlusion gate and the histogram of winning candidates under the
template mask.  Forward only: no autograd graph.  There is no CPU implementation.

    trk = WOFTChainedMulti(load_config("pytracking/configs/WOFT_chained_multi.py"))
    trk.init(frame0, [mask_a, mask_b, mask_c])
    Hs, metas = trk.track(frame1)

K planar targets on one dense track: the fold is shared, the planar stage is batched over the targets
(woft_chain_tc_multi, woft_tc_select_multi, woft_hfit_batched, woft_inlier_frac_batched, one read).
"""
import logging
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import ops, window
from .config import config_get, config_set
from .multiflow import MultiFlowTracker, _check_constants, _dev32
from .planar import BoundedCache, PlanarBuffers, decode, fit_and_judge
from .tracker import YAOFTrackerSingleControl, _count_components

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

    chain_photo_refine = N (absent, None or 0: off) runs the photometric refinement (woft_amd.photo; DESIGN.md sections 27, 29) on
    the pose of every frame that is not lost: W0 = inv(H_cur2init) against the template frame and the template mask on the whole
    current frame, N iterations at most; the pose becomes compose_H(inv(W)), meta.H_flow_cur2init keeps the fit's pose and
    meta.photo says what the refinement did (a lost frame has neither).  Its options: chain_photo_gain_bias, chain_photo_huber_k,
    chain_photo_stride, chain_photo_min_valid, chain_photo_eps, chain_photo_blur_sigma -- the parent's photo_* keys by meaning,
    default and error.

    chain_photo_weights = 'gate' or 'soft' (absent or None: off; it needs chain_photo_refine) weights that refinement by the
    frame's chain visibility: ONE woft_photo_weights launch per frame, right after the fold, turns the
    fold's cost and vis into a weight map on the template -- 1 ('gate') or exp(-cost) * vis ('soft') where the chain is valid and
    vis >= chain_vis_thr, 0 elsewhere, eroded by chain_photo_erode pixels (default 1, an integer 0 .. 4) -- and counts each
    target's mask pixels with a positive weight; the counts travel to pinned memory behind the launch and are read after the
    fit.  A target whose count / mask pixels is below chain_photo_min_support (default 0.25, a float in [0, 1]: a configurable
    default, not a tuned value) is not refined: it keeps the fit's pose and meta.photo.status is 'LOW_SUPPORT' (best -1, no
    iterates).  The others are refined with the map as the call's weights; meta.photo.support is the fraction and
    `photo_weight_map` the frame's map, a device tensor valid until the next track().  n_valid still counts in-frame pixels
    whatever their weight.

    A frame is lost when the fit is rejected (its H is still returned, the parent's `no_local_H` behaviour) or when fewer than
    4 correspondences survive or H is not finite (the previous pose is returned).  meta: lost, N_lost, global_H_success,
    H_global_cur2init (None when there was no usable fit), n_kept, chain_hist (int64 numpy, visible mask pixels per delta),
    chain_invalid, chain_occluded (mask pixels without a valid chain / with an occluded one)."""
    MASK_NEEDS_VISIBILITY_MODE = False            # ('weighted_masked' without a visibility_mode: the fold reads the mask)

    REFUSED_BY = "chained tracker"
    REFUSED = (
        ("visibility_mode", "the fold consumes the visibility mask of a 'weighted_masked' flow config itself (chain_vis_thr)"),
        ("fb_check", "the solver's one visibility slot carries the chains' occlusion gate"),
        ("warm_start_local", "there is no frame t-1 -> t stage to warm-start"),
        ("downscale_inputs", "the stored frames and results of the chains are kept at the input's size"),
        ("search_window_margin", "the chains read every pixel of every flow; the search-window tracker is WOFTWindow"),
        ("post_hoc_weights_postprocessing_fn", "the fit weight is exp(-chain cost), not a weight map to post-process"),
        ("photo_refine", "the chained trackers' pose has no per-frame template-to-frame stage to refine from (no pre-warp: the "
                         "chains carry the motion); the photometric refinement runs in YAOFTrackerSingleControl and WOFTWindow -- the chained "
                         "trackers refine their fitted pose under their own key, chain_photo_refine"),
    )

    def _refusals(self, config):
        super()._refusals(config)
        if config_set(config.flow_config, "weights_postprocessing_fn"):
            raise NotImplementedError("the chained tracker's chain cost is defined on the raw reliability logit; a flow config with "
                                      "a weights_postprocessing_fn is not supported")

    def __init__(self, config):
        self.chain_deltas = config_get(config, "chain_deltas", DEFAULT_DELTAS)
        self.chain_vis_thr = config_get(config, "chain_vis_thr", 0.5)
        self.chain_unit_cost = config_get(config, "chain_unit_cost", 1.0)
        self.chain_iters = config_get(config, "chain_iters", None)
        self.chain_weights = bool(config_get(config, "chain_weights", True))
        self.chain_share_features = bool(config_get(config, "chain_share_features", False))
        super().__init__(config)
        if not hasattr(self.flower, "pin_source"):
            raise NotImplementedError("the chained tracker needs this project's flow provider (pin_source, compute_flow(mode='flow', "
                                      f"borrow=True)); {type(self.flower).__name__} has no pin_source")
        self.multi = self._new_multi()            # (validates the chain keys)
        self.chain_deltas = self.multi.deltas
        self._photo = self._photo_config("chain_")    # (read once: None = off, and the frame's code path is what it is without it)
        self._photo_frame_of = (None, None)       # (frame number, the image the refinement reads of it)
        self.solver_decision += (f"; chained deltas {self.chain_deltas}; chain_share_features "
                                 f"{'on: every frame encoded once' if self.chain_share_features else 'off'}; pw_mask, no_prewarp_after_N, no_local_H and "
                                 "do_not_mask_TCs_by_prewarped are not used")
        if self._photo is not None:
            self.solver_decision += self._photo_decision("fitted")
        self._photo_w = self._photo_weights_config()
        self.photo_weight_map = None              # (the frame's weight map, a device tensor valid until the next track())
        self.photo_weights_wait_s = 0.0           # (seconds blocked on the support counts, also part of host_wait_s)
        self._pw = None
        if self._photo_w is not None:
            P = self._photo_w
            raft_type = self.flower.C.raft_type if hasattr(self.flower, "C") else config.flow_config.raft_type
            self.solver_decision += (f"; refinement weighted by chain visibility ({P['mode']}, vis >= {self.chain_vis_thr:.9g}, eroded by "
                                     f"{P['erode']}, targets under {P['min_support']:.9g} of their mask left at the fit's pose"
                                     + ("; raft_type 'orig' provides neither logit: the map only drops invalid chains"
                                        if raft_type == "orig" else "") + ")")
        if self._fused is not None and not self.chain_weights:
            self._fused = dict(self._fused, weighted=False)
        # the solver's visibility slot carries the chains' 0 / 1 occlusion gate, the way fb_check hands its verdict
        self._vis_mode, self._vis_thr = "gate", 0.5
        self._tc = BoundedCache()                 # grid size: the outputs of chain_tc, reused
        self._grid = BoundedCache()               # grid size: the (2, n) int64 source grid (callable back end only)

    def _new_multi(self):
        return MultiFlowTracker(self.flower, deltas=self.chain_deltas, vis_thr=self.chain_vis_thr, unit_cost=self.chain_unit_cost,
                                iters=self.chain_iters, share_features=self.chain_share_features)

    def _device_solver_reads(self, raft_type):
        return True                               # (weights and gate come from chain_tc, whatever the network provides)

    def _photo_weights_config(self):
        """-> None (off: `chain_photo_weights` absent or None) or dict(mode, erode, min_support) from chain_photo_weights ('gate' /
        'soft'), chain_photo_erode (1) and chain_photo_min_support (0.25: a configurable default, not a tuned value)."""
        C = self.C
        mode = config_get(C, "chain_photo_weights")
        if mode is None:
            return None
        if mode not in ops.PHOTO_WEIGHT_MODES:
            raise ValueError(f"chain_photo_weights {mode!r}: not None, 'gate' or 'soft'")
        if self._photo is None:
            raise ValueError("chain_photo_weights weights the photometric refinement: it needs chain_photo_refine, which is off")
        erode = config_get(C, "chain_photo_erode", 1)
        if isinstance(erode, bool) or not isinstance(erode, (int, np.integer)) or not 0 <= erode <= ops.PHOTO_WEIGHTS_MAX_RADIUS:
            raise ValueError(f"chain_photo_erode {erode!r}: not an integer in 0 .. {ops.PHOTO_WEIGHTS_MAX_RADIUS}")
        support = config_get(C, "chain_photo_min_support", 0.25)
        try:
            support = float(support)
        except (TypeError, ValueError):
            raise ValueError(f"chain_photo_min_support {support!r}: not a float in [0, 1]") from None
        if not (0.0 <= support <= 1.0):
            raise ValueError(f"chain_photo_min_support {support!r}: not a float in [0, 1]")
        return dict(mode=mode, erode=int(erode), min_support=support)

    def _init_photo_weights(self, bits, n_mask):
        """The per-tracker buffers of the weighting: the targets' (H, W) int32 bit plane, their masks' pixel counts, the device and
        pinned support counts and the event behind their copy."""
        if self._photo_w is None:
            return
        K = len(n_mask)
        self.photo_weight_map = None
        self._pw = SimpleNamespace(bits=bits, n_mask=[int(n) for n in n_mask], K=K, frame=None, fractions=None,
                                   map=torch.empty(tuple(bits.shape), dtype=torch.float32, device=self.device),
                                   support=torch.zeros(K, dtype=torch.int32, device=self.device),
                                   host=torch.zeros(K, dtype=torch.int32).pin_memory(), event=torch.cuda.Event())

    def _photo_weights_launch(self, out):
        """The frame's weight map and support counts from the fold result `out`: one launch, then the counts' asynchronous copy to
        pinned memory on the same stream -- enqueued before the planar stage, so that its read covers them."""
        W = self._pw
        if W is None:
            return
        h, w = (int(v) for v in W.bits.shape)
        rect = tuple(out.rect) if hasattr(out, "rect") else (0, 0, int(out.flow.shape[1]), int(out.flow.shape[2]))
        P = self._photo_w
        ops.photo_weights(out.cost, out.vis, rect, (h, w), W.bits, W.K, self.chain_vis_thr, ops.PHOTO_WEIGHT_MODES.index(P["mode"]),
                          P["erode"], W.map, W.support)
        W.host.copy_(W.support, non_blocking=True)
        W.event.record()
        W.frame, W.fractions, self.photo_weight_map = self._n_tracked, None, W.map

    def _photo_support(self, t):
        """Target t's support fraction of the frame being tracked (None: chain_photo_weights is off); the first call of a frame
        waits for the counts' copy -- it was enqueued before the planar stage's own read, so there is normally nothing to wait
        for -- and the wait is added to host_wait_s."""
        W = self._pw
        if W is None:
            return None
        if W.fractions is None:
            t0 = time.perf_counter()
            W.event.synchronize()
            waited = time.perf_counter() - t0
            self.host_wait_s += waited
            self.photo_weights_wait_s += waited
            counts = W.host.numpy()
            W.fractions = [float(counts[k]) / n if n else 0.0 for k, n in enumerate(W.n_mask)]
        return W.fractions[t]

    def _low_support(self, t):
        f = self._photo_support(t)
        return f is not None and f < self._photo_w["min_support"]

    def _wants_weights(self):
        return self.chain_weights and (self._fused is None or self._fused.get("weighted", True))

    def init(self, img, mask, img_identifier=None):
        super().init(img, mask, img_identifier)                      # (single-contour check, mask tensors, state: the parent's)
        self.multi = self._new_multi()
        self._init_multi(img)
        self._photo_frame_of = (None, None)
        if self._photo_w is not None:
            inside = self._template_mask_u8 != 0
            self._init_photo_weights(inside.to(torch.int32).contiguous(), [int(inside.sum())])
        # the chains read every pixel of every flow: no weight region, no flow region, no deferred weights
        if hasattr(self.flower, "pin_weight_region"):
            self.flower.pin_weight_region(None)
        if hasattr(self.flower, "pin_flow_region"):
            self.flower.pin_flow_region(None)
        self._sparse_weights = False

    def _init_multi(self, img):
        self.multi.init(img)                      # (the windowed tracker also names the template's rectangle here)

    def set_fast_meta(self, meta):
        raise NotImplementedError("Fastforward is not provided by the chained tracker: a replayed frame would leave a hole in the "
                                  "ring of stored frames the chains reach back to")

    def _source_grid(self, gh, gw):
        def make():
            i = torch.arange(gh * gw, device=self.device)
            return torch.stack([i % gw, torch.div(i, gw, rounding_mode="floor")])
        return self._grid.lookup((gh, gw), make)

    _SOLVE_ERRORS = (AssertionError,)             # what the planar stage turns into "no usable fit" (too few correspondences)

    def track(self, input_img, debug=False, img_identifier=None):
        self._n_tracked += 1
        out = self.multi.track(input_img, **self._begin_frame())      # (uploads the frame: the ring keeps a copy of its own)
        self._photo_weights_launch(out)
        H_cur2init, meta = self._planar_stage(self, out, input_img, img_identifier)
        self._after_frame([meta])
        return H_cur2init, meta

    # ---- what a tracker on search windows overrides: three hooks, the stages below are written once --------------------------------
    def _begin_frame(self):
        """Whatever the tracker settles before the frame's dense track -> what that track is given beside the frame."""
        return {}

    def _after_frame(self, metas):
        """After the frame's planar stage, with the meta of every target."""

    def _planes(self, out, input_img, state=None):
        """Where the planes of the fold result `out` lie, for the planar stage of `state` (None: of every target at once, on the bit
        plane) -> SimpleNamespace(
          origin:   None: whole frames, the stage goes through chain_tc / chain_tc_multi; else (y0, x0) of the planes' rectangle:
                    chain_tc_window / chain_tc_multi_window, whose gate holds the in-frame rule;
          frame_hw: the frame's size;  grid: the planes' size;
          mask, mask_hw: the uint8 mask or the bit plane to read (_frame_mask), laid out on the planes, and its size;
          bounds:   whether the selection checks the landings against mask_hw itself;
          crop_box: None, or the box the fit is taken back to frame coordinates from (H_undo_crop))."""
        hw = (int(input_img.shape[0]), int(input_img.shape[1]))
        return SimpleNamespace(origin=None, frame_hw=hw, grid=(int(out.flow.shape[1]), int(out.flow.shape[2])),
                               mask=self._frame_mask(state), mask_hw=hw, bounds=True, crop_box=None)

    def _frame_mask(self, state):
        return state._template_mask_u8

    def _planar_stage(self, state, out, input_img, img_identifier):
        """The fold result of one frame -> (H_cur2init, meta): correspondences, the fit, the update of `state` -- the holder of lost,
        N_lost, prev_H2init, last_good_H2init, _announced, n_kept and the mask _planes() names: the tracker, or a target of
        WOFTChainedMulti."""
        P = self._planes(out, input_img, state)
        fold = (out.flow, out.cost, out.vis, out.sel, P.mask, self.chain_vis_thr)
        kw = dict(want_w=self._wants_weights(), mask_hw=P.mask_hw, out=self._tc.get(P.grid))
        dst, w, ok, hist = self._tc.put(P.grid, ops.chain_tc(*fold, **kw) if P.origin is None
                                        else ops.chain_tc_window(*fold, P.origin, P.frame_hw, **kw))
        src_xy = None if self._fused is not None else self._source_grid(*P.grid)
        self.n_kept = None                                           # (the channel by which _solve reports the kept count)
        try:
            fit = self._solve(src_xy, dst, w, P.grid, P.mask_hw, P.mask, None, bounds=P.bounds, judge=True, vis=ok)
        except self._SOLVE_ERRORS:                                   # (too few correspondences for the estimator)
            fit = None
        if fit is not None and P.crop_box is not None:
            fit.H = window.H_undo_crop(P.crop_box, fit.H)
        state.n_kept = self.n_kept
        return self._finish(state, fit, hist.cpu().numpy().astype(np.int64), input_img, img_identifier)

    @staticmethod
    def _verdict(fit, n_kept):
        """-> (usable, success) of a frame's fit (None: there was none) with `n_kept` surviving correspondences."""
        usable = (fit is not None and not (n_kept is not None and n_kept < 4) and bool(np.all(np.isfinite(fit.H))))
        return usable, bool(usable and fit.success)

    @staticmethod
    def _photo_start(H_cur2init):
        """The refinement's start inv(H_cur2init), template -> frame; None where the pose has no finite inverse."""
        try:
            W0 = np.linalg.inv(H_cur2init)
        except np.linalg.LinAlgError:
            return None
        return W0 if np.all(np.isfinite(W0)) else None

    def _photo_frame(self, input_img):
        """The image the refinement reads of the frame being tracked, made once per frame whatever the number of targets."""
        if self._photo_frame_of[0] != self._n_tracked:
            self._photo_frame_of = (self._n_tracked, self._photo_image(input_img))
        return self._photo_frame_of[1]

    def _finish(self, state, fit, counts, input_img, img_identifier, photo=None):
        """A frame's fit (None: there was none), the target's `n_kept` and its histogram (int64 numpy) -> the update of `state`,
        (H_cur2init, meta).  photo: with chain_photo_refine, what a batched refinement returned for this target, (W, info) --
        (None, None) where it had no start; None: the refinement of `state`'s own template runs here."""
        meta = SimpleNamespace()
        n_kept = state.n_kept
        usable, success = self._verdict(fit, n_kept)
        meta.n_kept = n_kept
        meta.H_global_cur2init = fit.H.copy() if usable else None
        logger.debug(f"global_H_success: {success}")
        state.lost, state.N_lost = not success, (0 if success else state.N_lost + 1)
        # the fit maps current -> template; a rejected fit is still returned, no usable fit keeps the previous pose
        H_cur2init = fit.H if usable else state.prev_H2init
        if self._photo is not None and not state.lost:
            meta.H_flow_cur2init = H_cur2init.copy()                 # (the correspondence fit's pose, un-refined)
            target = getattr(state, "_target_index", 0)
            support = self._photo_support(target)                    # (None: chain_photo_weights is off)
            low = self._low_support(target)
            if photo is None:
                W0 = self._photo_start(H_cur2init)
                photo = (None, None)
                if W0 is not None and not low:
                    photo = state._photo_template.refine(self._photo_frame(input_img), W0, weights=self.photo_weight_map,
                                                         **self._photo_options())
                    self.host_wait_s += photo[1].host_wait_s
            meta.photo = None                                        # (no start: the pose stays what the fit gave)
            if low and self._photo_start(H_cur2init) is not None:    # (too little of the mask is visible: the fit's pose stays)
                meta.photo = SimpleNamespace(status="LOW_SUPPORT", best=-1, iterates=0, rms_before=float("nan"),
                                             rms_after=float("nan"), n_valid=0, gain=1.0, bias=0.0, support=support)
            elif photo[1] is not None:
                H_cur2init = self._photo_result(H_cur2init, photo[0], photo[1], meta)
                if support is not None:
                    meta.photo.support = support
        self.prev_img, self.prev_img_identifier = input_img, img_identifier
        self._set_pose(H_cur2init.copy(), good=not state.lost, state=state)
        meta.lost, meta.N_lost, meta.global_H_success = state.lost, state.N_lost, success
        meta.chain_hist = counts[:len(self.chain_deltas)].copy()
        meta.chain_invalid, meta.chain_occluded = int(counts[ops.CHAIN_HIST - 2]), int(counts[ops.CHAIN_HIST - 1])
        self._announce(meta, state)
        return H_cur2init.copy(), meta


MAX_TARGETS = ops.MULTI_MAX_TARGETS


def pack_target_bits(masks):
    """K (H, W) masks (anything numpy compares with 0; K <= 32, equal shapes) -> the (H, W) uint32 bit plane the multi-target
    kernels read: bit t of a pixel is set where masks[t] is non-zero there.  Masks may overlap."""
    if not 1 <= len(masks) <= MAX_TARGETS:
        raise ValueError(f"1 to {MAX_TARGETS} masks fit a bit plane, got {len(masks)}")
    bits = np.zeros(np.asarray(masks[0]).shape, np.uint32)
    for t, m in enumerate(masks):
        m = np.asarray(m)
        if m.shape != bits.shape:
            raise ValueError(f"mask {t}: shape {m.shape} differs from mask 0's {bits.shape}")
        bits |= (m != 0).astype(np.uint32) << np.uint32(t)
    return bits


class WOFTChainedMulti(WOFTChained):
    """K planar targets of one template frame on ONE chained dense track: nothing MultiFlowTracker computes
    depends on a template mask, so the K flows of a frame and their fold are shared and only the planar stage runs per target.

        trk.init(frame0, [mask_a, mask_b, mask_c])     # K = 1..32 masks (a list, or a (K, H, W) array); may overlap
        Hs, metas = trk.track(frame1)                  # Hs (K, 3, 3) float64; metas: a list of K namespaces

    Hs[t] and metas[t] are what a WOFTChained built from the same config returns when it is initialised with mask t alone and fed
    the same frames, bit for bit.  Each target has its own lost / N_lost / previous pose / last good pose: a target with fewer
    than 4 surviving correspondences or a non-finite fit keeps its previous pose and is lost, the others are not affected, and no
    exception of a target's fit leaves track().  Config keys and refusals are WOFTChained's.  Not provided: adding or removing a
    target after init(), autograd.  With chain_photo_refine the batched and select routes refine every target that is not lost in
    one PhotoTemplateMulti.refine call after the planar block's read (one call and one read more per frame, whatever K); the
    loop route refines per target with PhotoTemplate.

    The planar stage, by back end (`solver_decision` names the one in use; `meta.solver_decision` stays WOFTChained's text):
      device solver, Sobol draw, least-squares / IRLS estimator (the presets): chain_tc_multi, tc_select_multi, hfit_batched,
          inlier_frac_batched and one pinned read of one result block -- H (K, 9) | inlier fraction (K) | status (K) | selected and
          kept counts (2, K) | histograms (K, 130), 143 K words (woft_amd.planar: the one block of every tracker).  The number of
          launches and the one read do not depend on K.
      device solver with the RANSAC or the similarity (TRS) estimator: the same selection, then that estimator's single-element
          launch on each target's slices, inlier_frac_batched and the one read.
      device solver without a subsampler (counts can exceed the one-workgroup fit's 2048), or the config's own callables: a loop
          of WOFTChained's single-target stage over the targets' states and uint8 masks (K times its launches and reads)."""
    _SOLVE_ERRORS = (Exception,)                  # (a target's failed fit keeps that target's previous pose; nothing escapes)

    def __init__(self, config):
        super().__init__(config)
        self._single_decision = self.solver_decision
        F = self._fused
        if F is None or not F["n_draw"]:
            self._route = "loop"
            how = "a loop of the single-target stage (" + ("the config's own callables" if F is None else "no subsampler") + ")"
        elif F.get("ransac") is not None or F.get("trs") is not None:
            self._route = "select"
            how = ("one batched selection, the " + ("RANSAC" if F.get("ransac") is not None else "TRS")
                   + " estimator per target, one batched inlier test, one read")
        else:
            self._route = "batched"
            how = "one batched selection, one batched fit, one batched inlier test, one read"
        self.solver_decision += f"; multi-target planar stage: {how}"
        self._targets = []
        self._announced_targets = set()           # (as `_announced`: once per tracker, not once per init())

    def _decision_for_meta(self):
        return self._single_decision

    @staticmethod
    def _check_masks(img, masks):
        if isinstance(masks, torch.Tensor):
            masks = masks.detach().cpu().numpy()
        if isinstance(masks, np.ndarray):
            if masks.ndim != 3:
                raise ValueError(f"masks: a list of (H, W) masks or a (K, H, W) array is expected, got shape {masks.shape}")
            masks = list(masks)
        masks = [m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m) for m in masks]
        if not 1 <= len(masks) <= MAX_TARGETS:
            raise ValueError(f"init() takes 1 to {MAX_TARGETS} masks, got {len(masks)}")
        hw = (int(img.shape[0]), int(img.shape[1]))
        for t, m in enumerate(masks):
            if m.shape != hw:
                raise ValueError(f"target {t}: the mask's shape {m.shape} is not the frame's {hw}")
            if m.dtype not in (np.uint8, np.bool_):
                raise ValueError(f"target {t}: the mask's dtype {m.dtype} is not uint8 or bool")
        return masks

    def init(self, img, masks, img_identifier=None):
        masks = self._check_masks(img, masks)
        for t, m in enumerate(masks):
            assert _count_components(m > 0) == 1, f"target {t}: the mask is not a single contour"       # (the parent's check)
        super().init(img, masks[0], img_identifier)                  # (template, provider pins, the dense tracker: shared)
        eye = self.prev_H2init
        self._targets = [SimpleNamespace(lost=False, N_lost=0, prev_H2init=eye.copy(), last_good_H2init=eye.copy(),
                                         _announced=t in self._announced_targets, n_kept=None, _target_index=t,
                                         _template_mask_u8=torch.from_numpy((m > 0).astype(np.uint8) * 255).to(self.device))
                         for t, m in enumerate(masks)]
        self._tbits = torch.from_numpy(pack_target_bits(masks).view(np.int32)).to(self.device)
        self._init_photo_weights(self._tbits, [int(np.count_nonzero(m)) for m in masks])
        if self._photo is not None:
            from .photo import PhotoTemplate, PhotoTemplateMulti
            image, self._photo_template, self._photo_multi = self._photo_image(self.template_img), None, None
            if self._route == "loop":
                for T, m in zip(self._targets, masks):
                    T._photo_template = PhotoTemplate(image, m > 0, stride=self._photo["stride"])
            else:
                self._photo_multi = PhotoTemplateMulti(image, [m > 0 for m in masks], stride=self._photo["stride"])

    def _frame_mask(self, state):
        return self._tbits if state is None else super()._frame_mask(state)     # (None: every target at once, the bit plane)

    def _finish_batched(self, rows, input_img, img_identifier):
        """_finish for every target of a batched planar stage's rows; with chain_photo_refine the targets that are not lost go
        through ONE PhotoTemplateMulti.refine call (one launch sequence and one read whatever K) first."""
        photos = [None] * len(rows)
        if self._photo is not None:
            starts = [self._photo_start(fit.H) if self._verdict(fit, kept)[1] else None for fit, _, kept, _ in rows]
            # (with chain_photo_weights a target with too little visible support is passed as inactive)
            active = [W0 is not None and not self._low_support(t) for t, W0 in enumerate(starts)]
            photos = [(None, None)] * len(rows)
            if any(active):
                Ws, infos = self._photo_multi.refine(self._photo_frame(input_img),
                                                     np.stack([W0 if W0 is not None else np.eye(3) for W0 in starts]),
                                                     active=active, weights=self.photo_weight_map, **self._photo_options())
                waits = [i.host_wait_s for i in infos if i is not None]
                self.host_wait_s += max(waits) if waits else 0.0
                photos = [(W, info) if info is not None else (None, None) for W, info in zip(Ws, infos)]
        res = []
        for T, (fit, _, kept, counts), photo in zip(self._targets, rows, photos):
            T.n_kept = self.n_kept = kept
            res.append(self._finish(T, fit, counts, input_img, img_identifier, photo=photo))
        return res

    def track(self, input_img, debug=False, img_identifier=None):
        if not self._targets:
            raise RuntimeError(f"{type(self).__name__}.track() before init()")
        self._n_tracked += 1
        out = self.multi.track(input_img, **self._begin_frame())      # (the one dense track every target shares)
        self._photo_weights_launch(out)
        if self._route == "loop":
            res = [self._planar_stage(T, out, input_img, img_identifier) for T in self._targets]
        else:
            res = self._finish_batched(self._planar_batched(out, input_img), input_img, img_identifier)
        self._announced_targets.update(t for t, T in enumerate(self._targets) if T._announced)
        metas = [meta for _, meta in res]
        self._after_frame(metas)
        return np.stack([H for H, _ in res]), metas

    def _planar_batched(self, out, input_img):
        """The planar stage of every target on one fold result -> [(fit | None, selected, kept, histogram int64 numpy)] per
        target, the fits in frame coordinates.  chain_tc_multi's histograms land in the result block: one read."""
        F, K = self._fused, len(self._targets)
        P = self._planes(out, input_img)
        n_grid, cap, want_w = P.grid[0] * P.grid[1], 1024, self._wants_weights()     # (these routes have a Sobol draw: at most 1024 selected)
        blk = (b := self._buffers.lookup((K, n_grid, cap), lambda: PlanarBuffers(F, K, n_grid, cap, self.device, True, True))).block
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)
        tc = self._tc.lookup((K, n_grid), lambda: (new(2, n_grid), new(1, n_grid) if want_w else None, new(1, n_grid), blk.hist))
        fold = (out.flow, out.cost, out.vis, out.sel, P.mask, K, self.chain_vis_thr)
        kw = dict(want_w=want_w, mask_hw=P.mask_hw, out=tc)
        dst, w, ok, _ = (ops.chain_tc_multi(*fold, **kw) if P.origin is None
                         else ops.chain_tc_multi_window(*fold, P.origin, P.frame_hw, **kw))
        weighted = F.get("weighted", True)
        ops.tc_select_multi(dst, w if weighted else None, P.mask, K, *P.mask_hw, P.bounds, F["sobol_u"], ok, self._vis_mode,
                            self._vis_thr, b.ws, b.pa, b.pb, b.w, blk.count, grid=P.grid)
        fit_and_judge(F, b, weighted)
        self.host_wait_s += blk.read()
        res = decode(blk.host.numpy(), K, F, True)
        if P.crop_box is not None:
            for fit, _, _, _ in res:
                if fit is not None:
                    fit.H = window.H_undo_crop(P.crop_box, fit.H)
        return res
