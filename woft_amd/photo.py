"""Photometric refinement of a fitted homography on the device (csrc/photo.hip).

The fits of every other stage see flow correspondences at 1/8 resolution; this one looks at the pixels again: an
inverse-compositional Gauss-Newton alignment of the template's masked pixels to the frame, with an optional gain and bias, from
the pose a correspondence fit produced.  The semantics are this project's own (the reference has no such stage) and are stated
in include/woft_hip.h; a refinement is 2 (iters + 1) short launches enqueued back to back and ONE read of a result block -- no
host decision inside the loop.

    pt = PhotoTemplate(template, mask)                     # once per template
    H, info = pt.refine(frame, H_t2f)                      # per frame: H_t2f maps template pixels to frame pixels
    H, info = refine_homography(template, mask, frame, H_t2f)

    pm = PhotoTemplateMulti(template, [mask_a, mask_b])   # K targets of one template
    Hs, infos = pm.refine(frame, Hs_t2f, active=[True, True])     # one batched call and one read whatever K

    wmap, support = photo_weight_map(cost, vis, (h, w), bits=pm.bits, n_targets=pm.K)   # a fold result as weights (section 30)
    Hs, infos = pm.refine(frame, Hs_t2f, weights=wmap)                                   # ... of this call alone
"""
import math
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import ops

DEFAULTS = dict(iters=10, gain_bias=True, huber_k=None, min_valid=0.5, eps=1e-3)


def _device_image(img, what):
    """(H, W, 3) uint8 or float32, numpy or device tensor -> contiguous device tensor."""
    if isinstance(img, np.ndarray):
        if img.dtype not in (np.uint8, np.float32):
            raise TypeError(f"{what}: a uint8 or float32 image is expected, got {img.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(img))
    elif isinstance(img, torch.Tensor):
        if img.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f"{what}: a uint8 or float32 image is expected, got {img.dtype}")
        t = img
    else:
        raise TypeError(f"{what}: a numpy image or a device tensor is expected, got {type(img).__name__}")
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: shape (H, W, 3) is expected, got {tuple(t.shape)}")
    return (t if t.is_cuda else t.cuda()).contiguous()


def _h33(H, what):
    H = np.asarray(H, dtype=np.float64)
    if H.shape != (3, 3) or not np.all(np.isfinite(H)):
        raise ValueError(f"{what}: a finite 3x3 matrix is expected, got shape {H.shape}")
    return H


def check_options(iters, gain_bias, huber_k, min_valid, eps, prefix=""):
    """The refinement's options, checked and converted -> (iters, gain_bias, huber_k, min_valid, eps); ValueError names the key."""
    def bad(key, v, what):
        return ValueError(f"{prefix}{key} {v!r}: not {what}")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not (0 <= iters <= ops.PHOTO_MAX_ITERS):
        raise bad("iters", iters, f"an integer in 0 .. {ops.PHOTO_MAX_ITERS}")
    if huber_k is not None:
        try:
            hk = float(huber_k)
        except (TypeError, ValueError):
            raise bad("huber_k", huber_k, "None or a finite float > 0") from None
        if not (0.0 < hk < float("inf")):
            raise bad("huber_k", huber_k, "None or a finite float > 0")
        huber_k = hk
    try:
        mv, ep = float(min_valid), float(eps)
    except (TypeError, ValueError):
        raise bad("min_valid / eps", (min_valid, eps), "floats") from None
    if not (0.0 <= mv <= 1.0):
        raise bad("min_valid", min_valid, "a float in [0, 1]")
    if not (0.0 <= ep < float("inf")):
        raise bad("eps", eps, "a finite float >= 0")
    return int(iters), bool(gain_bias), huber_k, mv, ep


def _device_weights(weights, h, w, device):
    """The optional (h, w) float32 weight map, checked -> contiguous device tensor or None."""
    if weights is None:
        return None
    wt = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(weights))
    if tuple(wt.shape) != (h, w) or wt.dtype != torch.float32:
        raise ValueError(f"weights: float32 of shape {(h, w)} is expected, got {wt.dtype} {tuple(wt.shape)}")
    if bool((wt < 0).any()) or not bool(torch.isfinite(wt).all()):
        raise ValueError("weights: finite values >= 0 are expected")
    return wt.to(device).contiguous()


def _call_weights(own, weights, h, w, device):
    """The weight map of one call: `own` (the constructor's) when `weights` is None, else the per-call (h, w) float32 map.  A numpy
    map is checked as the constructor checks its own; a device tensor is checked for dtype, shape and device only -- scanning its
    values would synchronise the stream the map was just produced on (photo_weight_map's output is finite and >= 0 by
    construction)."""
    if weights is None:
        return own
    if not isinstance(weights, torch.Tensor) or not weights.is_cuda:
        return _device_weights(weights, h, w, device)
    if tuple(weights.shape) != (h, w) or weights.dtype != torch.float32:
        raise ValueError(f"weights: float32 of shape {(h, w)} is expected, got {weights.dtype} {tuple(weights.shape)}")
    if weights.device != device:
        raise ValueError(f"weights: a map on {device} is expected, got one on {weights.device}")
    return weights.contiguous()


def _pixel_set(inside, h, w, stride):
    """A boolean mask -> (box (x0, y0, x1, y1) inclusive, n_set, centre, scale) of its pixel set; (None, 0, None, None) when the
    mask is empty."""
    ys, xs = np.nonzero(inside)
    if not len(xs):
        return None, 0, None, None
    x0, x1, y0, y1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
    keep = ((xs >= 1) & (xs <= w - 2) & (ys >= 1) & (ys <= h - 2) & ((xs - x0) % stride == 0) & ((ys - y0) % stride == 0))
    return (x0, y0, x1, y1), int(keep.sum()), ((x0 + x1) / 2.0, (y0 + y1) / 2.0), max(x1 - x0, y1 - y0, 1) / 2.0


class _Result:
    """The device result block(s) of a refinement of `iters` iterations (one per target), the pinned host mirror and the event of
    the one read."""

    def __init__(self, iters, device, n_targets=1):
        n = n_targets * ops.PHOTO_REC * (iters + 2)
        self.dev = torch.zeros(n, dtype=torch.float64, device=device)
        self.host = torch.empty(n, dtype=torch.float64).pin_memory()
        self.event = torch.cuda.Event()

    def read(self):
        self.host.copy_(self.dev, non_blocking=True)
        self.event.record()
        t0 = time.perf_counter()
        self.event.synchronize()
        return time.perf_counter() - t0


class PhotoTemplate:
    """A template ((h, w, 3) uint8 or float32) and its mask ((h, w) uint8 or bool, > 0 inside), numpy or device tensors, prepared
    for refinements: the mask's bounding box, the normalisation, the pixel set's size `n_set` (mask > 0, not on the template's
    border, on the `stride` grid from the box's corner) and the device buffers.  weights: (h, w) float32 >= 0, optional."""

    def __init__(self, template, mask, stride=1, weights=None):
        if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1:
            raise ValueError(f"stride {stride!r}: not an integer >= 1")
        self.stride = int(stride)
        self.template = _device_image(template, "template")
        self.h, self.w = self.template.shape[:2]
        m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
        if m.shape != (self.h, self.w) or m.dtype not in (np.uint8, np.bool_):
            raise ValueError(f"mask: a uint8 or bool array of shape {(self.h, self.w)} is expected, got {m.dtype} {m.shape}")
        inside = m > 0
        self.mask = torch.from_numpy(np.ascontiguousarray(inside.astype(np.uint8))).to(self.template.device)
        self.weights = _device_weights(weights, self.h, self.w, self.template.device)
        self.box, self.n_set, centre, scale = _pixel_set(inside, self.h, self.w, self.stride)
        if self.box is not None:
            self.centre, self.scale = centre, scale
        self._results = {}

    def _launchable(self, nu):
        return self.box is not None and self.n_set >= nu and self.h >= 3 and self.w >= 3

    def normal_equations(self, frame, H_t2f, gain=1.0, bias=0.0, gain_bias=True, huber_k=None, weights=None):
        """One evaluation at the state (H_t2f, gain, bias in grey levels) -> (G (nu, nu), r (nu,), cost in grey levels, n_valid),
        float64 numpy; nu = 10 with gain_bias, else 8.  weights: as refine's."""
        _, gain_bias, huber_k, _, _ = check_options(0, gain_bias, huber_k, 0.5, 0.0)
        nu = 10 if gain_bias else 8
        if not self._launchable(nu):
            raise ValueError(f"the pixel set holds {self.n_set} pixels: fewer than the {nu} unknowns")
        frame = _device_image(frame, "frame")
        out = torch.empty(ops.PHOTO_NACC, dtype=torch.float64, device=self.template.device)
        ops.photo_eval(self.template, self.mask, _call_weights(self.weights, weights, self.h, self.w, self.template.device), frame, self.box, self.stride, _h33(H_t2f, "H_t2f"), float(gain),
                       3.0 * float(bias), gain_bias, huber_k, out)
        return unpack_sums(out.cpu().numpy(), nu)

    def refine(self, frame, H_t2f, iters=10, gain_bias=True, huber_k=None, min_valid=0.5, eps=1e-3, weights=None):
        """Refine H_t2f (3x3, template pixels -> frame pixels) against `frame` ((hf, wf, 3) uint8 or float32, numpy or device).
        weights: an (h, w) float32 map >= 0 that replaces the constructor's for this call (None: the constructor's).  A numpy map
        is checked as the constructor checks its own; a device tensor for dtype, shape and device only: scanning its values would
        synchronise.
        -> (H, info): H the best iterate's homography (h33 = 1; the input unchanged when no iterate was eligible), info with
        status ('CONVERGED', 'MAX_ITERS', 'TOO_FEW', 'SINGULAR', 'NONFINITE'), best (-1: none), the per-iterate arrays H_iter
        (k, 3, 3), gain, bias, cost (grey levels), n_valid, step (frame pixels; NaN where no step was taken), rms_before,
        rms_after, n_set and host_wait_s (the seconds blocked on the one read)."""
        iters, gain_bias, huber_k, min_valid, eps = check_options(iters, gain_bias, huber_k, min_valid, eps)
        H0 = _h33(H_t2f, "H_t2f")
        nu = 10 if gain_bias else 8
        weights = _call_weights(self.weights, weights, self.h, self.w, self.template.device)
        if not self._launchable(nu):                 # (an empty mask, or fewer pixels than unknowns: no launch)
            return H0.copy(), _info("TOO_FEW", -1, np.zeros((0, ops.PHOTO_REC)), self.n_set, 0.0)
        frame = _device_image(frame, "frame")
        res = self._results.get(iters)
        if res is None:
            res = self._results[iters] = _Result(iters, self.template.device)
        n_need = max(nu, int(math.ceil(min_valid * self.n_set)))
        ops.photo_refine(self.template, self.mask, weights, frame, self.box, self.stride, H0, iters, gain_bias, huber_k,
                         n_need, eps, res.dev)
        waited = res.read()
        blk = res.host.numpy()
        n_eval = int(blk[2])
        info = _info(ops.PHOTO_STATUS[int(blk[0])], int(blk[1]), blk[ops.PHOTO_REC:ops.PHOTO_REC * (1 + n_eval)]
                     .reshape(n_eval, ops.PHOTO_REC).copy(), self.n_set, waited)
        H = H0.copy() if info.best < 0 else blk[3:12].reshape(3, 3).copy()
        return H, info


class PhotoTemplateMulti:
    """K targets (1 .. 32) of ONE template for batched refinements against one frame: `masks` is a list of K
    (h, w) uint8 / bool masks or a (K, h, w) array, and may overlap.  Holds the targets' bit plane on the device (pack_target_bits'
    layout), per target the box, centre, scale and n_set by PhotoTemplate's rule, and one pinned result mirror per `iters`.
    Target t's results are PhotoTemplate(template, masks[t], stride, weights)'s, byte for byte."""

    def __init__(self, template, masks, stride=1, weights=None):
        from .chained import MAX_TARGETS, pack_target_bits
        if isinstance(masks, torch.Tensor):
            masks = masks.detach().cpu().numpy()
        if isinstance(masks, np.ndarray):
            if masks.ndim != 3:
                raise ValueError(f"masks: a list of (h, w) masks or a (K, h, w) array is expected, got shape {masks.shape}")
            masks = list(masks)
        masks = [m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m) for m in masks]
        if not 1 <= len(masks) <= MAX_TARGETS:
            raise ValueError(f"1 to {MAX_TARGETS} masks are expected, got {len(masks)}")
        if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1:
            raise ValueError(f"stride {stride!r}: not an integer >= 1")
        self.stride = int(stride)
        self.template = _device_image(template, "template")
        self.h, self.w = self.template.shape[:2]
        for t, m in enumerate(masks):
            if m.shape != (self.h, self.w) or m.dtype not in (np.uint8, np.bool_):
                raise ValueError(f"mask {t}: a uint8 or bool array of shape {(self.h, self.w)} is expected, got {m.dtype} {m.shape}")
        self.K = len(masks)
        self.weights = _device_weights(weights, self.h, self.w, self.template.device)
        self.bits = torch.from_numpy(pack_target_bits(masks).view(np.int32)).to(self.template.device)
        self.boxes, self.n_sets, self.centres, self.scales = [], [], [], []
        for m in masks:
            box, n_set, centre, scale = _pixel_set(m > 0, self.h, self.w, self.stride)
            self.boxes.append(box), self.n_sets.append(n_set), self.centres.append(centre), self.scales.append(scale)
        # (a target without a box never takes part; the entry points still check a box per target)
        self._call_boxes = [b if b is not None else (0, 0, 0, 0) for b in self.boxes]
        self._results = {}

    def _launchable(self, t, nu):
        return self.boxes[t] is not None and self.n_sets[t] >= nu and self.h >= 3 and self.w >= 3

    def _states(self, Hs):
        Hs = np.asarray(Hs, dtype=np.float64)
        if Hs.shape != (self.K, 3, 3) or not np.all(np.isfinite(Hs)):
            raise ValueError(f"Hs: finite matrices of shape {(self.K, 3, 3)} are expected, got shape {Hs.shape}")
        return Hs

    def _active(self, active, nu):
        if active is None:
            active = [True] * self.K
        if len(active) != self.K:
            raise ValueError(f"active: {self.K} entries are expected, got {len(active)}")
        active = [bool(a) for a in active]
        return active, [a and self._launchable(t, nu) for t, a in enumerate(active)]

    def normal_equations(self, frame, Hs, gains=None, biases=None, gain_bias=True, huber_k=None, weights=None):
        """One evaluation per target at the states (Hs (K, 3, 3), gains, biases in grey levels; None: 1 and 0) -> K tuples
        (G, r, cost, n_valid) as PhotoTemplate.normal_equations returns them.  weights: as PhotoTemplate.refine's, shared by the
        targets."""
        _, gain_bias, huber_k, _, _ = check_options(0, gain_bias, huber_k, 0.5, 0.0)
        nu = 10 if gain_bias else 8
        Hs = self._states(Hs)
        for t in range(self.K):
            if not self._launchable(t, nu):
                raise ValueError(f"target {t}: the pixel set holds {self.n_sets[t]} pixels: fewer than the {nu} unknowns")
        gains = [1.0] * self.K if gains is None else [float(g) for g in gains]
        biases = [0.0] * self.K if biases is None else [3.0 * float(b) for b in biases]
        frame = _device_image(frame, "frame")
        out = torch.empty((self.K, ops.PHOTO_NACC), dtype=torch.float64, device=self.template.device)
        ops.photo_eval_multi(self.template, self.bits, _call_weights(self.weights, weights, self.h, self.w, self.template.device), frame, self._call_boxes, self.stride, Hs, gains, biases,
                             [1] * self.K, gain_bias, huber_k, out)
        return [unpack_sums(row, nu) for row in out.cpu().numpy()]

    def refine(self, frame, Hs, active=None, iters=10, gain_bias=True, huber_k=None, min_valid=0.5, eps=1e-3, weights=None):
        """Refine the K poses Hs (K, 3, 3; template pixels -> frame pixels) against `frame` in ONE woft_photo_refine_multi call and
        ONE read -> (Hs_out (K, 3, 3) float64, infos): infos[t] is PhotoTemplate.refine's namespace; None and the input back for a
        target with active[t] false; 'TOO_FEW' with best = -1 and the input back, without taking part in the launch, for a target
        whose pixel set is empty or smaller than the unknowns.  No launch and no read when no target takes part.  weights: one
        (h, w) float32 map for this call, shared by the targets, checked as PhotoTemplate.refine checks its own; target t then gets
        the bytes of PhotoTemplate.refine(..., weights=weights) on its mask."""
        iters, gain_bias, huber_k, min_valid, eps = check_options(iters, gain_bias, huber_k, min_valid, eps)
        Hs = self._states(Hs)
        nu = 10 if gain_bias else 8
        weights = _call_weights(self.weights, weights, self.h, self.w, self.template.device)
        active, takes_part = self._active(active, nu)
        out = Hs.copy()
        infos = [None if not a else _info("TOO_FEW", -1, np.zeros((0, ops.PHOTO_REC)), self.n_sets[t], 0.0)
                 for t, a in enumerate(active)]
        if not any(takes_part):
            return out, infos
        frame = _device_image(frame, "frame")
        res = self._results.get(iters)
        if res is None:
            res = self._results[iters] = _Result(iters, self.template.device, self.K)
        n_need = [max(nu, int(math.ceil(min_valid * n))) for n in self.n_sets]
        ops.photo_refine_multi(self.template, self.bits, weights, frame, self._call_boxes, self.stride, Hs, n_need,
                               [int(a) for a in takes_part], iters, gain_bias, huber_k, eps, res.dev)
        waited = res.read()
        blocks = res.host.numpy().reshape(self.K, ops.PHOTO_REC * (iters + 2))
        for t, blk in enumerate(blocks):
            if not takes_part[t]:
                continue
            n_eval = int(blk[2])
            infos[t] = _info(ops.PHOTO_STATUS[int(blk[0])], int(blk[1]), blk[ops.PHOTO_REC:ops.PHOTO_REC * (1 + n_eval)]
                             .reshape(n_eval, ops.PHOTO_REC).copy(), self.n_sets[t], waited)
            if infos[t].best >= 0:
                out[t] = blk[3:12].reshape(3, 3)
        return out, infos


def unpack_sums(acc, nu):
    """The PHOTO_NACC doubles of one evaluation -> (G (nu, nu) symmetric, r, sqrt(cost) / 3, n_valid)."""
    tri = nu * (nu + 1) // 2
    G = np.zeros((nu, nu))
    G[np.triu_indices(nu)] = acc[:tri]
    G = G + np.triu(G, 1).T
    with np.errstate(all="ignore"):
        cost = float(np.sqrt(acc[tri + nu] / acc[tri + nu + 1]) / 3.0)
    return G, acc[tri:tri + nu].copy(), cost, int(acc[tri + nu + 2])


def _info(status, best, rec, n_set, waited):
    k = len(rec)
    cost = rec[:, 11].copy()
    return SimpleNamespace(status=status, best=best, H_iter=rec[:, :9].reshape(k, 3, 3).copy(), gain=rec[:, 9].copy(),
                           bias=rec[:, 10].copy(), cost=cost, n_valid=rec[:, 12].astype(np.int64), step=rec[:, 13].copy(),
                           rms_before=float(cost[0]) if k else float("nan"),
                           rms_after=float(cost[best]) if best >= 0 else float("nan"), n_set=n_set, host_wait_s=waited)


def refine_homography(template, mask, frame, H_t2f, stride=1, weights=None, **kw):
    """One-shot form: PhotoTemplate(template, mask, stride).refine(frame, H_t2f, weights=weights, **kw) -- a device map is passed
    through as refine takes it (dtype, shape and device checked, its values not read)."""
    if isinstance(weights, torch.Tensor) and weights.is_cuda:
        return PhotoTemplate(template, mask, stride=stride).refine(frame, H_t2f, weights=weights, **kw)
    return PhotoTemplate(template, mask, stride=stride, weights=weights).refine(frame, H_t2f, **kw)


def photo_weight_map(cost, vis, template_hw, rect=None, bits=None, n_targets=0, vis_thr=0.5, mode="gate", erode=1, out=None):
    """A fold result as the refinement's weight map (woft_photo_weights) -> (map (h, w) float32, support
    (n_targets,) int32 | None), both on the device, nothing read back.

    cost, vis:    the fold's planes (what MultiFlowTracker.track() returns, or chain_fold), fp32 tensors of rows * cols elements.
    template_hw:  (h, w) of the template the map is laid on.
    rect:         (ry, rx, rows, cols), where the planes lie in the template; None: origin (0, 0) and the planes' own 2-D size.
    bits:         the targets' bit plane (pack_target_bits' layout: an (h, w) uint32 numpy array, or its int32 device view) and
                  n_targets 1 .. 32; n_targets = 0: no support is computed and None is returned for it.
    vis_thr:      a pixel passes where its cost is finite and its vis >= vis_thr (equality passes, a NaN fails).
    mode:         'gate' -> 1.0 where the pixel passes; 'soft' -> exp(-cost) * vis in fp32 (0 where that is not finite or not > 0).
    erode:        the radius 0 .. 4 of the minimum over (2 erode + 1)^2 neighbours; neighbours outside the template are ignored,
                  neighbours inside the template but outside rect count as 0.
    out:          (map, support) of an earlier call of the same sizes, reused.
    support[t] counts the template pixels in target t whose map value is > 0: integer sums, so two calls give equal bytes."""
    h, w = (int(v) for v in template_hw)
    if not isinstance(cost, torch.Tensor) or not isinstance(vis, torch.Tensor):
        raise TypeError("photo_weight_map: cost and vis are tensors")
    if rect is None:
        shape = tuple(cost.shape[-2:]) if cost.dim() >= 2 else None
        if shape is None or cost.numel() != shape[0] * shape[1]:
            raise ValueError("photo_weight_map: without rect the cost plane must be (rows, cols) or (1, rows, cols)")
        rect = (0, 0) + shape
    try:
        ry, rx, rows, cols = (int(v) for v in rect)
    except (TypeError, ValueError):
        raise ValueError(f"photo_weight_map: rect is (ry, rx, rows, cols), got {rect!r}") from None
    if h < 1 or w < 1 or rows < 1 or cols < 1 or ry < 0 or rx < 0 or ry + rows > h or rx + cols > w:
        raise ValueError(f"photo_weight_map: rect {(ry, rx, rows, cols)} does not lie inside the template {(h, w)}")
    if cost.numel() != rows * cols or vis.numel() != rows * cols:
        raise ValueError(f"photo_weight_map: cost and vis must hold {rows} x {cols} elements")
    if mode not in ops.PHOTO_WEIGHT_MODES:
        raise ValueError(f"photo_weight_map: mode {mode!r} is not one of {ops.PHOTO_WEIGHT_MODES}")
    if isinstance(erode, bool) or not isinstance(erode, (int, np.integer)) or not 0 <= erode <= ops.PHOTO_WEIGHTS_MAX_RADIUS:
        raise ValueError(f"photo_weight_map: erode {erode!r} is not an integer in 0 .. {ops.PHOTO_WEIGHTS_MAX_RADIUS}")
    vis_thr = float(vis_thr)
    if not (0.0 <= vis_thr <= 1.0):
        raise ValueError(f"photo_weight_map: vis_thr must be in [0, 1], got {vis_thr!r}")
    if isinstance(n_targets, bool) or not isinstance(n_targets, (int, np.integer)) or not 0 <= n_targets <= ops.MULTI_MAX_TARGETS:
        raise ValueError(f"photo_weight_map: n_targets {n_targets!r} is not an integer in 0 .. {ops.MULTI_MAX_TARGETS}")
    n_targets = int(n_targets)
    if n_targets > 0 and bits is None:
        raise ValueError("photo_weight_map: n_targets > 0 needs the targets' bit plane")
    dev32 = lambda t: t.detach().to("cuda", torch.float32).contiguous()
    cost, vis = dev32(cost), dev32(vis)
    if n_targets > 0:
        if isinstance(bits, np.ndarray):
            if bits.dtype != np.uint32:
                raise ValueError(f"photo_weight_map: a numpy bit plane is uint32 (pack_target_bits), got {bits.dtype}")
            bits = torch.from_numpy(np.ascontiguousarray(bits).view(np.int32))
        if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int32 or tuple(bits.shape) != (h, w):
            raise ValueError(f"photo_weight_map: bits must be the {(h, w)} bit plane (uint32 numpy or its int32 tensor view)")
        bits = bits.to(cost.device).contiguous()
    if out is not None:
        wmap, support = out
    else:
        wmap = torch.empty((h, w), dtype=torch.float32, device=cost.device)
        support = torch.empty(n_targets, dtype=torch.int32, device=cost.device) if n_targets > 0 else None
    ops.photo_weights(cost, vis, (ry, rx, rows, cols), (h, w), bits, n_targets, vis_thr, ops.PHOTO_WEIGHT_MODES.index(mode), int(erode),
                      wmap, support)
    return wmap, support
