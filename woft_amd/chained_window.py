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
from .multiflow import MultiFlowTracker, _chain_fold, _rect

_EYE = np.eye(3)


def chain_fold_window(best, prev, step, k, template_rect, step_rect, post_H=None, vis_thr=0.5, unit_cost=1.0):
    """chain_fold on two rectangles -> (flow (2, rows, cols), cost, vis, sel (1, rows, cols)) on the template rectangle, new tensors
    on the device of the step's flow.

    template_rect: (y0, x0, rows, cols), the template rectangle that `best`, `prev` and the result are planes of.
    step_rect:     the rectangle of frames s and t the step's (2, rows, cols) flow and its logits cover.
    Flows are displacements in frame coordinates: q = template pixel + prev flow is looked up at q - (step origin) in the step's
    planes, and a q outside the step rectangle makes the candidate invalid.  post_H (3 x 3, optional): the candidate's landing
    pixel + flow is mapped through it in fp64 before the flow is stored (the inverse of a pre-warp of frame t); a landing with a
    non-positive denominator is invalid.  Everything else -- best, prev, step, k, the key, ties, host tensors -- as chain_fold."""
    return _chain_fold("chain_fold_window", best, prev, step, k, vis_thr, unit_cost, rects=(template_rect, step_rect), post_H=post_H)


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

    # ---- WOFTChained's hooks: track() and the planar stages are the whole-frame trackers' ----------------------------------------
    def _begin_frame(self):
        """Settles the pre-warp of the direct candidate (None: chain_prewarp is off): last_good_H2init, reset to the identity
        here once the tracker has been lost for more than no_prewarp_after_N frames."""
        if not self.chain_prewarp:
            return dict(prewarp_H=None)
        if self.C.no_prewarp_after_N and self.N_lost > self.C.no_prewarp_after_N:
            self.last_good_H2init = _EYE.copy()
        return dict(prewarp_H=self.last_good_H2init)

    def _after_frame(self, metas):
        self._follow()
        for meta in metas:
            meta.chain_window = self.chain_window

    def _planes(self, out, input_img, state=None):
        """R0's planes: the stage runs in R0's coordinates on the mask cropped to R0 (_window_mask); woft_chain_tc_window's gate
        holds the in-frame rule, so the selection checks no bounds; the fit is un-cropped where R0 does not start at the frame's
        origin."""
        y0, x0, gh, gw = out.rect
        mask = self._window_mask(state)
        return SimpleNamespace(origin=(y0, x0), frame_hw=(int(input_img.shape[0]), int(input_img.shape[1])), grid=(gh, gw), mask=mask,
                               mask_hw=tuple(int(v) for v in mask.shape), bounds=False,
                               crop_box=self._R0_box if (y0, x0) != (0, 0) else None)

    def _window_mask(self, state):
        return state._mask_crop                  # (`state` also holds its mask's crop to R0: the tracker, or a target)

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
