"""The multi-target chained tracker on search windows: K planar targets of one template frame on ONE chained dense track whose flows
run on ONE window, the union of the targets' boxes plus a margin.  DESIGN.md section 28.

    trk = WOFTChainedMultiWindow(load_config("pytracking/configs/WOFT_chained_multi_window.py"))
    trk.init(frame0, [mask_a, mask_b, mask_c])
    Hs, metas = trk.track(frame1)          # Hs (K, 3, 3); metas[t].chain_window: the one window named for the frame

WOFTChainedMulti's sharing (one set of flows and one fold per frame, whatever K is) with WOFTChainedWindow's rectangles (flows on
the tracked planes' box instead of on whole frames).  Forward only: no autograd graph.  There is no CPU implementation.
"""
import numpy as np
import torch

from . import ops, window
from .chained import WOFTChainedMulti
from .chained_window import WOFTChainedWindow
from .config import config_get

_EYE = np.eye(3)


class WOFTChainedMultiWindow(WOFTChainedMulti, WOFTChainedWindow):
    """WOFTChainedMulti whose dense tracker is a WindowedMultiFlowTracker (this project's own).  The template rectangle is
    R0 = chain_rect(union of the K template masks' boxes, ...), fixed at init(); the bit plane of the masks is cropped to R0 once.
    After each frame every target's template mask is carried by inv(its prev_H2init) -- ONE woft_mask_bbox_multi launch and one read
    of 5 K ints; none when every pose is the identity -- and B_t = chain_rect(union of the contributing boxes) names the window of
    the flows that will start at this frame.  A target with an identity pose contributes its template box; one with a singular or
    non-finite pose, or with nothing set in its carried mask, contributes nothing; with no contributor the previous window stays.

    init(), track(), the per-target state, the announcements and "a failing target keeps its pose and disturbs nobody" are
    WOFTChainedMulti's; meta.chain_window of every target, and the tracker's chain_window, is the one shared window.  With one mask
    the results are WOFTChainedWindow's (chain_prewarp off) byte for byte; with a falsy margin they are WOFTChainedMulti's.

    track() and both planar stages are inherited unchanged: WOFTChainedWindow's hooks (_begin_frame, _after_frame, _planes) tell them
    where the planes lie, and _after_frame calls the _follow below.  The planar stage runs in R0's coordinates, by WOFTChainedMulti's
    routes:
      batched: chain_tc_multi_window, tc_select_multi without a bounds check on the cropped bit plane (the gate already holds the
          in-frame rule), hfit_batched, inlier_frac_batched, one pinned read of the one result block, H_undo_crop per target on the
          host where R0's origin is not (0, 0).
      select:  the same selection, then the RANSAC or TRS estimator per target.
      loop:    the single-target stage per target, on the per-target uint8 mask crops.
    Launches and reads of the batched route do not depend on K: the planar block's read, plus at most one box read.

    Config keys: WOFTChainedWindow's (search_window_margin, chain_window_quantum, chain_window_min) and WOFTChainedMulti's.
    chain_share_features is refused with WOFTChainedWindow's reason.  chain_prewarp defaults to False and True is refused: the
    pre-warp of the direct candidate is one pose, K targets have K.  Not provided: a window per target, adding or removing a target
    after init(), autograd."""
    PREWARP_DEFAULT = False

    def _refusals(self, config):
        super()._refusals(config)
        if config_get(config, "chain_prewarp", False):
            raise NotImplementedError("chain_prewarp is not provided by the multi-target windowed chained tracker: the pre-warp of the "
                                      "direct candidate is one pose, and K targets have K poses")

    def __init__(self, config):
        super().__init__(config)
        self.solver_decision += f"; one union search window for all targets (planar stage on the window's planes, route '{self._route}')"
        self._masks_in = None
        self._tbits_crop = None

    # ---- init ---------------------------------------------------------------------------------------------------------------------
    def init(self, img, masks, img_identifier=None):
        self._masks_in = self._check_masks(img, masks)
        try:
            super().init(img, self._masks_in, img_identifier)        # (-> _init_multi below, then the targets and the bit plane)
            for T, m in zip(self._targets, self._masks_in):
                T._template_box = window.Box.from_mask(m > 0)
        finally:
            self._masks_in = None
        R0, (Hh, Ww) = self.chain_window, self._frame_hw
        whole = R0 == (0, 0, Hh, Ww)
        # the bit plane on R0: four bytes a pixel through the byte crop
        self._tbits_crop = self._tbits if whole else (ops.crop_u8(self._tbits.view(torch.uint8).reshape(Hh, Ww, 4), R0)
                                                      .view(torch.int32).reshape(R0[2], R0[3]))
        if self._route == "loop":
            for T in self._targets:
                T._mask_crop = T._template_mask_u8 if whole else ops.crop_u8(T._template_mask_u8, R0)

    def _init_multi(self, img):
        """The dense tracker on R0 = chain_rect(union of the template masks' boxes)."""
        boxes = [window.Box.from_mask(m > 0) for m in self._masks_in]
        self._frame_hw = tuple(int(v) for v in self._masks_in[0].shape)
        R0 = self._chain_rect(window.union_box(boxes), self._frame_hw)
        self.multi.init(img, R0)
        self.chain_window = R0
        self._R0_box = window.Box(R0[1], R0[0], R0[3], R0[2])

    def _window_mask(self, state):
        return self._tbits_crop if state is None else super()._window_mask(state)     # (None: every target at once)

    # ---- the window of the frame just tracked -------------------------------------------------------------------------------------
    def _follow(self):
        """Name the one window of the frame just tracked: every target's template mask carried by inv(its prev_H2init), the union
        of the contributing boxes, chain_rect."""
        if not self._margin:
            return                                                   # (whole frames: the window never moves)
        boxes, carry = [None] * len(self._targets), [None] * len(self._targets)
        for t, T in enumerate(self._targets):
            if np.array_equal(T.prev_H2init, _EYE):
                boxes[t] = T._template_box                           # (the identity: the template's own box, no warp)
                continue
            try:
                to_frame = np.linalg.inv(T.prev_H2init)
                back = np.linalg.inv(to_frame)                       # (what the launch warps by: it refuses a non-finite entry)
            except np.linalg.LinAlgError:
                continue
            if np.all(np.isfinite(to_frame)) and np.all(np.isfinite(back)):
                carry[t] = to_frame
        if any(Hm is not None for Hm in carry):
            rows = ops.mask_bbox_multi(self._tbits, len(self._targets), carry).cpu().tolist()
            for t, (rmin, rmax, cmin, cmax, any_set) in enumerate(rows):
                if carry[t] is not None and any_set:
                    boxes[t] = window.Box.from_extent(rmin, rmax, cmin, cmax)
        box = window.union_box(boxes)
        if box is not None:                                          # (else: the previous frame's window)
            self.chain_window = self._chain_rect(box, self._frame_hw)
        self.multi.set_rect(self.chain_window)
