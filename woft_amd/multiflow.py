"""Multi-delta chained dense tracking on the HIP fold kernel of csrc/flow_multi.hip.  DESIGN.md section 18.

Follow every pixel of a template frame through a video: per frame t and per temporal stride delta, the stored result
template -> (t - delta) is chained with the flow (t - delta) -> t, and per pixel the most reliable chain is kept -- the one with
the smallest key (occluded, cost), where cost sums softplus(-reliability logit) along the chain and the visibility is the product
of the steps' sigmoid(visibility logit).

    flow, cost, vis, sel = chain_fold(None, None, (flow_0t, wlogit_0t), k=0)             # the direct candidate
    flow, cost, vis, sel = chain_fold((flow, cost, vis, sel), prev, (flow_st, wlogit_st), k=1)

    trk = MultiFlowTracker(provider)
    trk.init(frame0)
    out = trk.track(frame1)            # out.flow (2, H, W), out.cost, out.vis, out.occluded, out.sel (1, H, W), out.frame_index

Forward only: no autograd graph.  There is no CPU implementation of the fold.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import ops

MAX_DELTAS, MAX_DELTA = 8, 127


def _dev32(t, what, n=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: a torch tensor is expected, got {type(t).__name__}")
    if not t.is_floating_point():
        raise TypeError(f"{what}: a floating-point tensor is expected, got {t.dtype}")
    if n is not None and t.numel() != n:
        raise ValueError(f"{what}: {n} elements are expected, got a tensor of shape {tuple(t.shape)}")
    return t.detach().to(device="cuda", dtype=torch.float32).contiguous()


def _check_constants(vis_thr, unit_cost):
    vis_thr, unit_cost = float(vis_thr), float(unit_cost)
    if not (0.0 <= vis_thr <= 1.0):
        raise ValueError(f"vis_thr must be in [0, 1], got {vis_thr!r}")
    if not (unit_cost >= 0.0):
        raise ValueError(f"unit_cost must be >= 0, got {unit_cost!r}")
    return vis_thr, unit_cost


def _rect(rect, what):
    try:
        y0, x0, rows, cols = (int(v) for v in rect)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a rectangle is (y0, x0, rows, cols), got {rect!r}") from None
    if y0 < 0 or x0 < 0 or rows <= 0 or cols <= 0:
        raise ValueError(f"{what}: origin >= 0 and sides >= 1 are expected, got {rect!r}")
    return y0, x0, rows, cols


def _chain_fold(name, best, prev, step, k, vis_thr, unit_cost, rects=None, post_H=None):
    """The one body of chain_fold and chain_fold_window (`name`: the caller's, for messages): best / prev / step / k checked and
    normalised to contiguous fp32 device tensors, the fold, the result on the device of the step's flow.  rects: None (whole
    frames: every plane has the step flow's size) or (template_rect, step_rect)."""
    vis_thr, unit_cost = _check_constants(vis_thr, unit_cost)
    k = int(k)
    if not 0 <= k <= MAX_DELTA:
        raise ValueError(f"{name}: k must be in [0, {MAX_DELTA}], got {k}")
    if rects is not None:
        trect, srect = _rect(rects[0], "template_rect"), _rect(rects[1], "step_rect")
    step = tuple(step) if isinstance(step, (tuple, list)) else (step,)
    if not 1 <= len(step) <= 3:
        raise ValueError(f"{name}: step is (flow,), (flow, wlogit) or (flow, wlogit, mlogit)")
    sflow = step[0]
    if rects is None:
        if not isinstance(sflow, torch.Tensor) or sflow.dim() != 3 or sflow.shape[0] != 2:
            raise ValueError(f"{name}: the step's flow must be a (2, H, W) tensor")
        (h, w), (sh, sw) = sflow.shape[1:], sflow.shape[1:]
    else:
        (h, w), (sh, sw) = trect[2:], srect[2:]
        if not isinstance(sflow, torch.Tensor) or tuple(sflow.shape) != (2, sh, sw):
            raise ValueError(f"{name}: the step's flow must be a (2, {sh}, {sw}) tensor, the step rectangle's size")
    n, ns = h * w, sh * sw
    f = _dev32(sflow, "step flow")
    logits = [None if t is None else _dev32(t, "step logit", ns) for t in (step + (None, None))[1:3]]
    if prev is not None:
        if len(prev) != 3:
            raise ValueError(f"{name}: prev is None or (flow, cost, vis)")
        prev = (_dev32(prev[0], "prev flow", 2 * n).reshape(2, h, w), _dev32(prev[1], "prev cost", n), _dev32(prev[2], "prev vis", n))
    if best is not None:
        if len(best) != 4 or best[3].dtype != torch.int32 or best[3].numel() != n:
            raise ValueError(f"{name}: best is None or (flow, cost, vis, sel int32)")
        # (clones: the fold is in place, the caller's tensors stay as they are)
        best = (_dev32(best[0], "best flow", 2 * n).reshape(2, h, w).clone(), _dev32(best[1], "best cost", n).clone(),
                _dev32(best[2], "best vis", n).clone(), best[3].detach().to("cuda").contiguous().clone())
    common = dict(k=k, vis_thr=vis_thr, unit_cost=unit_cost, first=best is None)
    if rects is None:
        bf, bc, bv, bs = ops.flow_chain_fold(best, prev, f, logits[0], logits[1], **common)
    else:
        bf, bc, bv, bs = ops.flow_chain_fold_window(best, prev, f, logits[0], logits[1], template_rect=trect, step_rect=srect,
                                                    post_H=post_H, **common)
    dev = sflow.device
    return bf.to(dev), bc.reshape(1, h, w).to(dev), bv.reshape(1, h, w).to(dev), bs.reshape(1, h, w).to(dev)


def chain_fold(best, prev, step, k, vis_thr=0.5, unit_cost=1.0):
    """Fold one candidate chain into a running per-pixel best -> (flow (2, H, W), cost (1, H, W), vis (1, H, W),
    sel (1, H, W) int32), new tensors on the device of the step's flow.

    best: None (this candidate starts the fold) or the (flow, cost, vis, sel) of the folds so far; it is not modified.
    prev: None (the chain starts at the template itself: flow 0, cost 0, vis 1) or (flow, cost, vis) of template -> s.
    step: (flow,), (flow, wlogit) or (flow, wlogit, mlogit) of s -> t; a None logit, or a shorter tuple, means the step costs
          `unit_cost` / is fully visible.  The logits are raw: no sigmoid, no post-processing.
    k:    the candidate's index in [0, 127], stored in sel where the candidate wins.
    Per pixel: q = pixel + prev flow; flow = prev flow + step flow(q); cost = prev cost + softplus(-wlogit(q));
    vis = prev vis * sigmoid(mlogit(q)), all sampled with the edge-exact bilinear sampler of chain_flow.  A candidate whose q
    leaves the frame, or that meets a non-finite value, is invalid and replaces nothing.  The candidate replaces the best where
    the best is empty, or occluded (vis < vis_thr) while the candidate is not, or equally occluded and strictly dearer: ties keep
    the earlier fold.  A pixel without any valid candidate has flow NaN, cost +inf, vis 0, sel -1.
    Host tensors are copied to the device and the result is handed back on their device.  Computed in fp32."""
    return _chain_fold("chain_fold", best, prev, step, k, vis_thr, unit_cost)


class MultiFlowTracker:
    """Dense long-term tracking of every template pixel by chaining flows over several temporal strides.

    provider: a RAFTWrapper of any raft_type -- 'orig' gives neither logit (every step costs `unit_cost` and is visible),
              'weighted' the reliability logit, 'weighted_masked' both.
    deltas:   the candidates of a frame, in fold order (ties go to the earlier one): None = the direct flow template -> t, an
              int d = the stored result of frame t - d chained with the flow (t - d) -> t.  Non-empty, unique, at most 8 entries,
              each int in [1, 127].
    iters:    the refinement iterations of every flow (None: the flow config's).
    share_features: encode every frame once (provider.encode_frame) and run its flows from the record -- as the target of the
              K flows of its own frame, and as the source of the chained flows of later frames -- instead of from the image:
              one fnet and one cnet pass per frame, where the default runs K fnet passes over the frame and an fnet and a cnet
              pass per chained flow over a stored one.  The results are bit-identical.  The records are kept beside the ring in
              `_records` and dropped with their ring entries: 4 * P * (fdim + hdim + cdim) bytes per stored frame on top of
              the frame and its result, P = (padded height / 8) * (padded width / 8) -- 66.4 MB at 1080p on the full model, 2.1 GB
              for the 32 frames the default deltas keep.  The template's direct flow keeps the pinned source.  Default off."""
    DEVICE = "cuda"

    def __init__(self, provider, deltas=(None, 1, 2, 4, 8, 16, 32), vis_thr=0.5, unit_cost=1.0, iters=None, share_features=False):
        try:
            deltas = tuple(deltas)
        except TypeError:
            raise ValueError(f"deltas must be a sequence of None / positive ints, got {deltas!r}") from None
        if not 1 <= len(deltas) <= MAX_DELTAS:
            raise ValueError(f"deltas must have 1 to {MAX_DELTAS} entries, got {len(deltas)}")
        for d in deltas:
            if d is not None and (isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 1 <= d <= MAX_DELTA):
                raise ValueError(f"deltas: each entry is None or an int in [1, {MAX_DELTA}], got {d!r}")
        deltas = tuple(None if d is None else int(d) for d in deltas)
        if len(set(deltas)) != len(deltas):
            raise ValueError(f"deltas must be unique, got {deltas!r}")
        self.vis_thr, self.unit_cost = _check_constants(vis_thr, unit_cost)
        if iters is not None and (isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 1):
            raise ValueError(f"iters must be None or an int >= 1, got {iters!r}")
        if getattr(getattr(provider, "C", None), "weights_postprocessing_fn", None):
            raise NotImplementedError("MultiFlowTracker: the chain cost is defined on the raw reliability logit; a flow config "
                                      "with a weights_postprocessing_fn is not supported")
        self.share_features = bool(share_features)
        if self.share_features and not hasattr(provider, "encode_frame"):
            raise NotImplementedError("MultiFlowTracker(share_features=True) needs a flow provider with encode_frame() and "
                                      f"compute_flow() on its records; {type(provider).__name__} has no encode_frame")
        self.provider, self.deltas, self.iters = provider, deltas, None if iters is None else int(iters)
        self.reach = max([d for d in deltas if d is not None], default=0)     # how far back a stored frame can still be needed
        self._fold = ops.flow_chain_fold
        self.reset()

    def reset(self):
        """Forget the template and every stored frame."""
        self._template, self._ring, self.frame_index = None, {}, None
        self._records = {}                                  # share_features: frame index -> its FrameFeatures, beside _ring

    def _upload(self, frame):
        """-> an (H, W, 3) uint8 tensor of the tracker's own on the device (never a view of the caller's or the provider's)."""
        t = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frame))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise TypeError(f"frames are (H, W, 3) uint8 BGR images, got {tuple(t.shape)} {t.dtype}")
        return t.detach().to(self.DEVICE, copy=True).contiguous()

    def init(self, frame):
        """Frame 0: the template.  It is pinned in the provider (its features are computed once) and stored with the identity
        result -- flow 0, cost 0, vis 1."""
        self.reset()
        self._template = self._upload(frame)
        self.provider.pin_source(self._template)
        self.frame_index = 0
        if self.reach:
            h, w = self._out_size(self._template)
            z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.DEVICE)
            self._ring[0] = (self._template, (z(2, h, w), z(h, w), torch.ones(h, w, dtype=torch.float32, device=self.DEVICE)))
            if self.share_features:                         # (a chained flow from frame 0 starts from its record, like any other)
                self._records[0] = self.provider.encode_frame(self._template)

    def _out_size(self, img):
        """(H, W) of the provider's flow maps for this frame size (padding_mode 'crop' trims the frame to multiples of 8)."""
        h, w = int(img.shape[0]), int(img.shape[1])
        if getattr(getattr(self.provider, "C", None), "padding_mode", None) == "crop":
            h, w = h // 8 * 8, w // 8 * 8
        return h, w

    def _empty(self, h, w):
        """The result of a frame that no candidate reaches: flow NaN, cost +inf, vis 0, sel -1 everywhere."""
        full = lambda v, dtype, *s: torch.full(s, v, dtype=dtype, device=self.DEVICE)
        return (full(float("nan"), torch.float32, 2, h, w), full(float("inf"), torch.float32, h, w),
                full(0.0, torch.float32, h, w), full(-1, torch.int32, h, w))

    def schedule(self, t):
        """The candidates of frame t -> [(k, source frame index, chained)]: k indexes `deltas`; chained = False for the direct
        candidate (no stored result is read).  A delta reaching before frame 0 has no candidate."""
        return [(k, 0 if d is None else t - d, d is not None) for k, d in enumerate(self.deltas) if d is None or t - d >= 0]

    def track(self, frame):
        """The next frame -> SimpleNamespace(flow (2, H, W), cost (1, H, W), vis (1, H, W), occluded (1, H, W) bool,
        sel (1, H, W) int32 = the index into `deltas` of the winning chain (-1: none was valid), frame_index): where each
        template pixel is in this frame.  Tensors of the caller's own."""
        if self._template is None:
            raise RuntimeError("MultiFlowTracker.track() before init()")
        t = self.frame_index + 1
        img = self._upload(frame)
        extra = {} if self.iters is None else dict(iters=self.iters)
        best = None
        sched = self.schedule(t)
        # share_features: the frame is encoded once, here (even where a single flow reads it: its record is a later frame's source)
        rec = self.provider.encode_frame(img) if self.share_features and (sched or self.reach) else None
        for k, s, chained in sched:
            src, prev = self._ring[s] if chained else (self._template, None)
            if rec is not None and chained:
                src = self._records[s]
            out = self.provider.compute_flow(src, img if rec is None else rec, mode="flow", do_sigmoid=False, borrow=True, **extra)
            flow, wl, ml = out[0], out[1], (out[2] if len(out) > 2 else None)
            # (the borrowed buffers are consumed here, before the next flow overwrites them)
            best = self._fold(best, prev, flow, wl, ml, k=k, vis_thr=self.vis_thr, unit_cost=self.unit_cost, first=best is None)
        if best is None:                                   # (every delta reaches before frame 0)
            best = self._empty(*self._out_size(img))
        bf, bc, bv, bs = best
        h, w = bf.shape[1:]
        self.frame_index = t
        if self.reach:
            self._ring[t] = (img, (bf, bc, bv))
            if rec is not None:
                self._records[t] = rec
            for old in [i for i in self._ring if i < t + 1 - self.reach]:      # (frame t + 1 reaches back to t + 1 - reach)
                del self._ring[old]
                self._records.pop(old, None)
        return SimpleNamespace(flow=bf.clone(), cost=bc.reshape(1, h, w).clone(), vis=bv.reshape(1, h, w).clone(),
                               occluded=(bv < self.vis_thr).reshape(1, h, w), sel=bs.reshape(1, h, w), frame_index=t)
