"""The chained trackers on search windows: flows on rectangles that follow the object, folded by the rectangle form of the fold
kernel (woft_flow_chain_fold_window, csrc/flow_multi.hip).  DESIGN.md section 26.

    flow, cost, vis, sel = chain_fold_window(None, None, (flow_0t, wlogit_0t), 0, template_rect=R0, step_rect=R0)
    flow, cost, vis, sel = chain_fold_window((flow, cost, vis, sel), prev, (flow_st, wlogit_st), 1, template_rect=R0, step_rect=B_s)

    trk = WindowedMultiFlowTracker(provider)
    trk.init(frame0, R0)               # R0 = (y0, x0, rows, cols): the template rectangle every result lives on
    out = trk.track(frame1)            # MultiFlowTracker's namespace on R0's planes, plus out.rect
    trk.set_rect(B_1)                  # where the object is in frame 1: the window of the flows that start there

    trk = WOFTChainedWindow(load_config("pytracking/configs/WOFT_chained_window.py"))
    trk.init(frame0, mask)
    H_cur2init, meta = trk.track(frame1)

A rectangle is (y0, x0, rows, cols) in frame pixels, as woft_amd.window.chain_rect gives it.  Forward only: no autograd graph.
There is no CPU implementation.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import ops, window
from .chained import WOFTChained
from .config import config_get
from .multiflow import MAX_DELTA, MultiFlowTracker, _check_constants, _dev32

_EYE = np.eye(3)


def _rect(rect, what):
    try:
        y0, x0, rows, cols = (int(v) for v in rect)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a rectangle is (y0, x0, rows, cols), got {rect!r}") from None
    if y0 < 0 or x0 < 0 or rows <= 0 or cols <= 0:
        raise ValueError(f"{what}: origin >= 0 and sides >= 1 are expected, got {rect!r}")
    return y0, x0, rows, cols


def chain_fold_window(best, prev, step, k, template_rect, step_rect, post_H=None, vis_thr=0.5, unit_cost=1.0):
    """chain_fold on two rectangles -> (flow (2, rows, cols), cost, vis, sel (1, rows, cols)) on the template rectangle, new tensors
    on the device of the step's flow.

    template_rect: (y0, x0, rows, cols), the template rectangle that `best`, `prev` and the result are planes of.
    step_rect:     the rectangle of frames s and t the step's (2, rows, cols) flow and its logits cover.
    Flows are displacements in frame coordinates: q = template pixel + prev flow is looked up at q - (step origin) in the step's
    planes, and a q outside the step rectangle makes the candidate invalid.  post_H (3 x 3, optional): the candidate's landing
    pixel + flow is mapped through it in fp64 before the flow is stored (the inverse of a pre-warp of frame t); a landing with a
    non-positive denominator is invalid.  Everything else -- best, prev, step, k, the key, ties, host tensors -- as chain_fold."""
    vis_thr, unit_cost = _check_constants(vis_thr, unit_cost)
    k = int(k)
    if not 0 <= k <= MAX_DELTA:
        raise ValueError(f"chain_fold_window: k must be in [0, {MAX_DELTA}], got {k}")
    ty0, tx0, th, tw = _rect(template_rect, "template_rect")
    sy0, sx0, sh, sw = _rect(step_rect, "step_rect")
    step = tuple(step) if isinstance(step, (tuple, list)) else (step,)
    if not 1 <= len(step) <= 3:
        raise ValueError("chain_fold_window: step is (flow,), (flow, wlogit) or (flow, wlogit, mlogit)")
    sflow = step[0]
    if not isinstance(sflow, torch.Tensor) or tuple(sflow.shape) != (2, sh, sw):
        raise ValueError(f"chain_fold_window: the step's flow must be a (2, {sh}, {sw}) tensor, the step rectangle's size")
    n, ns = th * tw, sh * sw
    f = _dev32(sflow, "step flow")
    logits = [None if t is None else _dev32(t, "step logit", ns) for t in (step + (None, None))[1:3]]
    if prev is not None:
        if len(prev) != 3:
            raise ValueError("chain_fold_window: prev is None or (flow, cost, vis)")
        prev = (_dev32(prev[0], "prev flow", 2 * n).reshape(2, th, tw), _dev32(prev[1], "prev cost", n), _dev32(prev[2], "prev vis", n))
    if best is not None:
        if len(best) != 4 or best[3].dtype != torch.int32 or best[3].numel() != n:
            raise ValueError("chain_fold_window: best is None or (flow, cost, vis, sel int32)")
        # (clones: the fold is in place, the caller's tensors stay as they are)
        best = (_dev32(best[0], "best flow", 2 * n).reshape(2, th, tw).clone(), _dev32(best[1], "best cost", n).clone(),
                _dev32(best[2], "best vis", n).clone(), best[3].detach().to("cuda").contiguous().clone())
    bf, bc, bv, bs = ops.flow_chain_fold_window(best, prev, f, logits[0], logits[1], k=k, template_rect=(ty0, tx0, th, tw),
                                                step_rect=(sy0, sx0, sh, sw), post_H=post_H, vis_thr=vis_thr, unit_cost=unit_cost,
                                                first=best is None)
    dev = sflow.device
    return bf.to(dev), bc.reshape(1, th, tw).to(dev), bv.reshape(1, th, tw).to(dev), bs.reshape(1, th, tw).to(dev)


class WindowedMultiFlowTracker(MultiFlowTracker):
    """MultiFlowTracker whose flows run on rectangles: the template rectangle R0, fixed at init(), and per stored frame s the
    rectangle B_s that set_rect() named after frame s was tracked (R0 when it was not called).

    The direct candidate is the flow from the template's crop by R0 to R0 of the frame; a chained candidate from frame s the flow
    from the stored crop of frame s by B_s to the same rectangle B_s of the frame, chained onto the stored result template -> s
    where that result lands inside B_s.  Results live on R0's planes (flows in frame coordinates).  The ring keeps, per frame,
    its crop by its rectangle and its result on R0: 3 |B_s| + 16 |R0| bytes, not 19 bytes per frame pixel.  (The last frame is
    held whole until its rectangle is known: until set_rect() or the next track().)  deltas, vis_thr, unit_cost, iters:
    MultiFlowTracker's.  share_features is not offered: the crops of one frame differ per flow, there is no one encoding to share.
    The provider is told to keep len(deltas) + 1 plans beside the pinned one (bound_plans) where it can be told."""

    def __init__(self, provider, deltas=(None, 1, 2, 4, 8, 16, 32), vis_thr=0.5, unit_cost=1.0, iters=None):
        super().__init__(provider, deltas=deltas, vis_thr=vis_thr, unit_cost=unit_cost, iters=iters, share_features=False)
        self._fold = ops.flow_chain_fold_window
        if hasattr(provider, "bound_plans"):
            provider.bound_plans(len(self.deltas) + 1)

    def reset(self):
        super().reset()
        self.rect0 = None                    # R0 with the sides of the provider's flow maps: the rectangle of every result
        self._R0 = None                      # R0 as given (the crop's rectangle)
        self._hw = None                      # the frames' (H, W)
        self._pending = None                 # (frame index, whole frame, result): the last frame, until its rectangle is known
        self._pending_rect = None            # ... and the rectangle it gets when nobody names one: R0

    def _crop(self, img, rect):
        """The tracker's own crop of `img` by rect; the whole frame is handed through (it is the tracker's own upload already)."""
        if rect[:2] == (0, 0) and rect[2:] == tuple(img.shape[:2]):
            return img
        return ops.crop_u8(img, rect)

    def _fit(self, rect, img, what):
        y0, x0, rows, cols = _rect(rect, what)
        if y0 + rows > img.shape[0] or x0 + cols > img.shape[1]:
            raise ValueError(f"{what}: {rect!r} leaves the {tuple(img.shape[:2])} frame")
        return y0, x0, rows, cols

    def init(self, frame, rect):
        """Frame 0 and the template rectangle R0.  The template's crop is pinned in the provider; frame 0 is stored with the
        identity result on R0 -- flow 0, cost 0, vis 1 -- and, until set_rect() says otherwise, with the rectangle R0."""
        self.reset()
        img = self._upload(frame)
        self._hw = tuple(int(v) for v in img.shape[:2])
        self._R0 = self._fit(rect, img, "init: rect")
        self._template = self._crop(img, self._R0)
        self.provider.pin_source(self._template)
        h, w = self._out_size(self._template)
        self.rect0 = self._R0[:2] + (h, w)
        self.frame_index = 0
        if self.reach:
            z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.DEVICE)
            self._pending = (0, img, (z(2, h, w), z(h, w), torch.ones(h, w, dtype=torch.float32, device=self.DEVICE)))
            self._pending_rect = self._R0

    def set_rect(self, rect):
        """Name the source window of the frame just tracked (or of frame 0, after init()): the rectangle its chained flows to
        later frames run on.  The frame's crop enters the ring; the whole frame is let go."""
        if self._template is None:
            raise RuntimeError("WindowedMultiFlowTracker.set_rect() before init()")
        if self._pending is None:
            if self.reach:
                raise RuntimeError("set_rect(): the rectangle of this frame has been named already")
            return
        self._pending_rect = self._fit(rect, self._pending[1], "set_rect")
        self._seal()

    def _seal(self):
        """The pending frame enters the ring as (crop, rectangle, result on R0)."""
        if self._pending is None:
            return
        t, img, res = self._pending
        rect = self._pending_rect
        # (frame 0 by R0 is the pinned template crop itself, as MultiFlowTracker's ring holds its pinned template)
        crop = self._template if (t == 0 and rect == self._R0) else self._crop(img, rect)
        self._ring[t] = (crop, rect, res)
        self._pending = None
        for old in [i for i in self._ring if i < t + 1 - self.reach]:          # (frame t + 1 reaches back to t + 1 - reach)
            del self._ring[old]

    def track(self, frame, prewarp_H=None):
        """The next frame -> MultiFlowTracker.track()'s namespace on R0's planes, plus rect = (y0, x0, rows, cols) of those planes.
        prewarp_H (3 x 3, optional): the direct candidate runs to R0 of the frame warped by it (woft_warp_perspective_window_u8)
        and its landings go back through inv(prewarp_H) in the fold; None or the identity: the frame's own pixels."""
        if self._template is None:
            raise RuntimeError("WindowedMultiFlowTracker.track() before init()")
        self._seal()
        t = self.frame_index + 1
        img = self._upload(frame)
        if tuple(img.shape[:2]) != self._hw:
            raise ValueError(f"track: a {tuple(img.shape[:2])} frame after an init() frame of {self._hw}")
        extra = {} if self.iters is None else dict(iters=self.iters)
        post_H = None
        if prewarp_H is not None and not np.array_equal(np.asarray(prewarp_H, dtype=np.float64), _EYE):
            post_H = np.linalg.inv(np.asarray(prewarp_H, dtype=np.float64))
            post_H = post_H / post_H[2, 2]
        best = None
        for k, s, chained in self.schedule(t):
            if chained:
                src, rect, prev = self._ring[s]
                dst, pH = self._crop(img, rect), None
            else:
                src, rect, prev, pH = self._template, self._R0, None, post_H
                if pH is None:
                    dst = self._crop(img, rect)
                else:
                    dst = torch.empty_like(self._template)
                    ops.warp_perspective_window_u8(img, prewarp_H, rect, dst, None)
            out = self.provider.compute_flow(src, dst, mode="flow", do_sigmoid=False, borrow=True, **extra)
            flow, wl, ml = out[0], out[1], (out[2] if len(out) > 2 else None)
            # (the borrowed buffers are consumed here, before the next flow overwrites them)
            best = self._fold(best, prev, flow, wl, ml, k=k, template_rect=self.rect0,
                              step_rect=rect[:2] + tuple(int(v) for v in flow.shape[1:]), post_H=pH, vis_thr=self.vis_thr,
                              unit_cost=self.unit_cost, first=best is None)
        h, w = self.rect0[2:]
        if best is None:                                   # (every delta reaches before frame 0)
            best = self._empty(h, w)
        bf, bc, bv, bs = best
        self.frame_index = t
        if self.reach:
            self._pending, self._pending_rect = (t, img, (bf, bc, bv)), self._R0
        return SimpleNamespace(flow=bf.clone(), cost=bc.reshape(1, h, w).clone(), vis=bv.reshape(1, h, w).clone(),
                               occluded=(bv < self.vis_thr).reshape(1, h, w), sel=bs.reshape(1, h, w), frame_index=t, rect=self.rect0)


class WOFTChainedWindow(WOFTChained):
    """WOFTChained on search windows (this project's own): the chained flows run on the tracked plane's box plus a margin instead
    of on whole frames.  R0 = chain_rect(template mask's box, ...) is the rectangle of the template the chains live on; after each
    frame the template mask is carried by inv(prev_H2init) (one woft_mask_bbox launch and its 20-byte read; none for an identity
    pose), its box goes through chain_rect and names the window B_t of the flows that will start at this frame.  A singular pose,
    or a carried mask with nothing set, keeps the previous frame's window.

    Config keys beside WOFTChained's: search_window_margin (falsy: whole frames -- then, with chain_prewarp off, the results are
    WOFTChained's byte for byte), chain_window_quantum (64), chain_window_min (window.MIN_WINDOW), chain_prewarp (True: the direct
    candidate runs to the frame pre-warped by last_good_H2init, reset to the identity after `no_prewarp_after_N` lost frames as
    YAOFTrackerSingleControl does).  chain_share_features is refused.  meta.chain_window is the window named for the frame.
    The planar stage runs in R0's coordinates on woft_chain_tc_window's correspondences (whose gate already holds the in-frame
    rule) and the fit is taken back to frame coordinates by H_undo_crop where R0's origin is not (0, 0)."""
    REFUSED_BY = "windowed chained tracker"
    REFUSED = tuple(r for r in WOFTChained.REFUSED if r[0] != "search_window_margin") + (
        ("chain_share_features", "the crops of one frame differ per flow: there is no one encoding of a frame to share"),
    )
    PREWARP_DEFAULT = True                        # (chain_prewarp when the config does not name it)

    def __init__(self, config):
        self._margin = config_get(config, "search_window_margin", None) or None       # (absent key: an empty, falsy Config)
        self.chain_window_quantum = window.check_quantum(config_get(config, "chain_window_quantum", 64))
        self.chain_window_min = config_get(config, "chain_window_min", window.MIN_WINDOW)
        self.chain_prewarp = bool(config_get(config, "chain_prewarp", self.PREWARP_DEFAULT))
        super().__init__(config)
        self.solver_decision += (f"; chained flows on search windows (margin {self._margin}, quantum {self.chain_window_quantum}, "
                                 f"pre-warped direct flow {'on' if self.chain_prewarp else 'off'})")
        self.chain_window = None

    def _new_multi(self):
        return WindowedMultiFlowTracker(self.flower, deltas=self.chain_deltas, vis_thr=self.chain_vis_thr,
                                        unit_cost=self.chain_unit_cost, iters=self.chain_iters)

    def _chain_rect(self, box, hw):
        return window.chain_rect(box, self._margin, hw[1], hw[0], self.chain_window_quantum, self.chain_window_min)

    def _init_multi(self, img):
        inside = self.np_template_mask > 0
        self._frame_hw = inside.shape
        self._template_box = window.Box.from_mask(inside)
        R0 = self._chain_rect(self._template_box, inside.shape)
        self.multi.init(img, R0)
        self.chain_window = R0
        self._R0_box = window.Box(R0[1], R0[0], R0[3], R0[2])
        self._mask_crop = ops.crop_u8(self._template_mask_u8, R0)

    def track(self, input_img, debug=False, img_identifier=None):
        self._n_tracked += 1
        prewarp_H = None
        if self.chain_prewarp:
            if self.C.no_prewarp_after_N and self.N_lost > self.C.no_prewarp_after_N:
                self.last_good_H2init = _EYE.copy()
            prewarp_H = self.last_good_H2init
        out = self.multi.track(input_img, prewarp_H=prewarp_H)           # (uploads the frame: the ring keeps crops of its own)
        self._photo_weights_launch(out)                                  # (R0's planes placed in the full template frame)
        H_cur2init, meta = self._planar_stage(self, out, input_img, img_identifier)
        self._follow()
        meta.chain_window = self.chain_window
        return H_cur2init, meta

    def _planar_stage(self, state, out, input_img, img_identifier):
        """WOFTChained's stage in R0's coordinates: woft_chain_tc_window's gate holds the in-frame rule, so the selection checks
        no bounds; the fit is un-cropped where R0 does not start at the frame's origin.  `state` also holds _mask_crop: the
        tracker, or a target of WOFTChainedMultiWindow."""
        Hh, Ww = int(input_img.shape[0]), int(input_img.shape[1])
        y0, x0, gh, gw = out.rect
        mask, mask_hw = state._mask_crop, tuple(int(v) for v in state._mask_crop.shape)
        dst, w, ok, hist = self._tc.put((gh, gw), ops.chain_tc_window(out.flow, out.cost, out.vis, out.sel, mask, self.chain_vis_thr,
                                                                      (y0, x0), (Hh, Ww), want_w=self._wants_weights(),
                                                                      mask_hw=mask_hw, out=self._tc.get((gh, gw))))
        src_xy = None if self._fused is not None else self._source_grid(gh, gw)
        self.n_kept = None                                           # (the channel by which _solve reports the kept count)
        try:
            fit = self._solve(src_xy, dst, w, (gh, gw), mask_hw, mask, None, bounds=False, judge=True, vis=ok)
        except self._SOLVE_ERRORS:                                   # (too few correspondences for the estimator)
            fit = None
        if fit is not None and (y0, x0) != (0, 0):
            fit.H = window.H_undo_crop(self._R0_box, fit.H)
        state.n_kept = self.n_kept
        return self._finish(state, fit, hist.cpu().numpy().astype(np.int64), input_img, img_identifier)

    def _follow(self):
        """Name the window of the frame just tracked: the template mask carried by inv(prev_H2init), its box, chain_rect."""
        if not self._margin:
            return                                                   # (whole frames: the window never moves)
        box = self._template_box
        if not np.array_equal(self.prev_H2init, _EYE):
            try:
                to_frame = np.linalg.inv(self.prev_H2init)
            except np.linalg.LinAlgError:
                to_frame = None
            if to_frame is None or not np.all(np.isfinite(to_frame)):
                box = None
            else:
                rmin, rmax, cmin, cmax, any_set = ops.mask_bbox(self._template_mask_u8, Hmat=to_frame).cpu().tolist()
                box = window.Box.from_extent(rmin, rmax, cmin, cmax) if any_set else None
        if box is not None:                                          # (else: the previous frame's window)
            self.chain_window = self._chain_rect(box, self._frame_hw)
        self.multi.set_rect(self.chain_window)
