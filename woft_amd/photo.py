"""Photometric refinement of a fitted homography on the device (csrc/photo.hip).

The fits of every other stage see flow correspondences at 1/8 resolution; this one looks at the pixels again: an
inverse-compositional Gauss-Newton alignment of the template's masked pixels to the frame, with an optional gain and bias, from
the pose a correspondence fit produced.  The semantics are this project's own (the reference has no such stage) and are stated
in include/woft_hip.h; a refinement is 2 (iters + 1) short launches enqueued back to back and ONE read of a result block -- no
host decision inside the loop.

    pt = PhotoTemplate(template, mask)                     # once per template
    H, info = pt.refine(frame, H_t2f)                      # per frame: H_t2f maps template pixels to frame pixels
    H, info = refine_homography(template, mask, frame, H_t2f)
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


class _Result:
    """The device result block of a refinement of `iters` iterations, its pinned host mirror and the event of its one read."""

    def __init__(self, iters, device):
        n = ops.PHOTO_REC * (iters + 2)
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
        self.weights = None
        if weights is not None:
            wt = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(weights))
            if tuple(wt.shape) != (self.h, self.w) or wt.dtype != torch.float32:
                raise ValueError(f"weights: float32 of shape {(self.h, self.w)} is expected, got {wt.dtype} {tuple(wt.shape)}")
            if bool((wt < 0).any()) or not bool(torch.isfinite(wt).all()):
                raise ValueError("weights: finite values >= 0 are expected")
            self.weights = wt.to(self.template.device).contiguous()
        ys, xs = np.nonzero(inside)
        self.box, self.n_set = None, 0
        if len(xs):
            x0, x1, y0, y1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
            self.box = (x0, y0, x1, y1)
            keep = ((xs >= 1) & (xs <= self.w - 2) & (ys >= 1) & (ys <= self.h - 2)
                    & ((xs - x0) % self.stride == 0) & ((ys - y0) % self.stride == 0))
            self.n_set = int(keep.sum())
            self.centre = ((x0 + x1) / 2.0, (y0 + y1) / 2.0)
            self.scale = max(x1 - x0, y1 - y0, 1) / 2.0
        self._results = {}

    def _launchable(self, nu):
        return self.box is not None and self.n_set >= nu and self.h >= 3 and self.w >= 3

    def normal_equations(self, frame, H_t2f, gain=1.0, bias=0.0, gain_bias=True, huber_k=None):
        """One evaluation at the state (H_t2f, gain, bias in grey levels) -> (G (nu, nu), r (nu,), cost in grey levels, n_valid),
        float64 numpy; nu = 10 with gain_bias, else 8."""
        _, gain_bias, huber_k, _, _ = check_options(0, gain_bias, huber_k, 0.5, 0.0)
        nu = 10 if gain_bias else 8
        if not self._launchable(nu):
            raise ValueError(f"the pixel set holds {self.n_set} pixels: fewer than the {nu} unknowns")
        frame = _device_image(frame, "frame")
        out = torch.empty(ops.PHOTO_NACC, dtype=torch.float64, device=self.template.device)
        ops.photo_eval(self.template, self.mask, self.weights, frame, self.box, self.stride, _h33(H_t2f, "H_t2f"), float(gain),
                       3.0 * float(bias), gain_bias, huber_k, out)
        return unpack_sums(out.cpu().numpy(), nu)

    def refine(self, frame, H_t2f, iters=10, gain_bias=True, huber_k=None, min_valid=0.5, eps=1e-3):
        """Refine H_t2f (3x3, template pixels -> frame pixels) against `frame` ((hf, wf, 3) uint8 or float32, numpy or device).
        -> (H, info): H the best iterate's homography (h33 = 1; the input unchanged when no iterate was eligible), info with
        status ('CONVERGED', 'MAX_ITERS', 'TOO_FEW', 'SINGULAR', 'NONFINITE'), best (-1: none), the per-iterate arrays H_iter
        (k, 3, 3), gain, bias, cost (grey levels), n_valid, step (frame pixels; NaN where no step was taken), rms_before,
        rms_after, n_set and host_wait_s (the seconds blocked on the one read)."""
        iters, gain_bias, huber_k, min_valid, eps = check_options(iters, gain_bias, huber_k, min_valid, eps)
        H0 = _h33(H_t2f, "H_t2f")
        nu = 10 if gain_bias else 8
        if not self._launchable(nu):                 # (an empty mask, or fewer pixels than unknowns: no launch)
            return H0.copy(), _info("TOO_FEW", -1, np.zeros((0, ops.PHOTO_REC)), self.n_set, 0.0)
        frame = _device_image(frame, "frame")
        res = self._results.get(iters)
        if res is None:
            res = self._results[iters] = _Result(iters, self.template.device)
        n_need = max(nu, int(math.ceil(min_valid * self.n_set)))
        ops.photo_refine(self.template, self.mask, self.weights, frame, self.box, self.stride, H0, iters, gain_bias, huber_k,
                         n_need, eps, res.dev)
        waited = res.read()
        blk = res.host.numpy()
        n_eval = int(blk[2])
        info = _info(ops.PHOTO_STATUS[int(blk[0])], int(blk[1]), blk[ops.PHOTO_REC:ops.PHOTO_REC * (1 + n_eval)]
                     .reshape(n_eval, ops.PHOTO_REC).copy(), self.n_set, waited)
        H = H0.copy() if info.best < 0 else blk[3:12].reshape(3, 3).copy()
        return H, info


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
    """One-shot form: PhotoTemplate(template, mask, stride, weights).refine(frame, H_t2f, **kw)."""
    return PhotoTemplate(template, mask, stride=stride, weights=weights).refine(frame, H_t2f, **kw)
