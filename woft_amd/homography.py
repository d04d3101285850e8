"""Homography estimators with the reference's operator API
(/root/reference/pytracking/utils/least_squares_H.py): same function names, argument meaning,
return shapes and AssertionError behaviour; the arithmetic runs in the HIP fit kernels
(csrc/hfit.hip) on the device the points live on.
"""
import numpy as np
import torch

from . import ops
from .probe import recorder


class _Probe:
    """Sentinel passed through user re-weighting callables to recognise the built-in losses."""


def IRLSq_L1(residuals, eps=1e-8):
    """least_squares_H.py:268-269."""
    if isinstance(residuals, _Probe):
        return ("l1", 0.0, eps)
    return 1 / (torch.abs(residuals) + eps)


def IRLSq_Huber(residuals, k=1, eps=1e-8):
    """L2 up to +-k, then L1 (least_squares_H.py:272-277)."""
    if isinstance(residuals, _Probe):
        return ("huber", float(k), eps)
    abs_res = torch.abs(residuals)
    weights = 1 / (abs_res + eps)
    weights[abs_res < k] = 1
    return weights


def _check(points1, points2):
    if points1.shape != points2.shape:
        raise AssertionError(points1.shape)
    if not (len(points1.shape) >= 1 and points1.shape[-1] == 2):
        raise AssertionError(points1.shape)
    if points1.shape[1] < 4:
        raise AssertionError(points1.shape)


def _operands(points1, points2, weights, b):
    pa = points1[b].float().contiguous()
    pb = points2[b].float().contiguous()
    w = weights[b].float().reshape(-1).contiguous() if weights is not None else None
    if w is not None and w.numel() != pa.shape[0]:
        raise AssertionError(weights.shape)
    return pa, pb, w


def _launch(points1, points2, weights, reweight, huber_k, n_irls):
    """The fit of device tensors: one woft_hfit_batched launch for B > 1 and N <= HFIT_SINGLE_MAX, else woft_hfit per element."""
    B, N = points1.shape[0], points1.shape[1]
    out = torch.empty(B, 3, 3, dtype=torch.float32, device=points1.device)
    status = torch.zeros(B, dtype=torch.int32, device=points1.device)
    if B > 1 and N <= ops.HFIT_SINGLE_MAX:
        # one launch, one workgroup per element (woft_hfit_batched): the bits of the per-element loop below
        pa, pb = points1.float().contiguous(), points2.float().contiguous()
        w = weights.float().reshape(B, -1).contiguous() if weights is not None else None
        if w is not None and w.shape[1] != N:
            raise AssertionError(weights.shape)
        ops.hfit_batched(pa, pb, w, out, status, reweight=reweight, huber_k=huber_k, n_irls=n_irls)
        return out
    for b in range(B):
        pa, pb, w = _operands(points1, points2, weights, b)
        ops.hfit(pa, pb, w, out[b].view(9), status[b:b + 1], reweight=reweight, huber_k=huber_k, n_irls=n_irls)
    return out


class _WeightedLSqFit(torch.autograd.Function):
    """The plain weighted fit with a backward (csrc/hfit.hip hfit_batched_bwd_kernel).  forward makes the
    launches of _launch, so H has the bits of the call without grad; backward is one launch that recomputes the small solve and
    writes the gradients of the inputs that need one.  Once differentiable.  An element whose fit failed (NaN H) gets ZERO
    gradients, where torch autograd through a QR would give NaN: one degenerate sample must not poison an optimiser step whose
    loss masks it out."""

    @staticmethod
    def forward(ctx, points1, points2, weights):
        ctx.save_for_backward(points1, points2, weights)
        return _launch(points1.detach(), points2.detach(), None if weights is None else weights.detach(), 0, 0.0, 0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        points1, points2, weights = ctx.saved_tensors
        B, N = points1.shape[0], points1.shape[1]
        pa, pb = points1.float().contiguous(), points2.float().contiguous()
        w = weights.float().reshape(B, -1).contiguous() if weights is not None else None
        gH = grad_output.to(torch.float32).contiguous().view(B, 9)
        need = ctx.needs_input_grad
        gpa = torch.empty_like(pa) if need[0] else None
        gpb = torch.empty_like(pb) if need[1] else None
        gw = torch.empty_like(w) if (need[2] and w is not None) else None
        ops.hfit_batched_bwd(pa, pb, w, gH, gpa, gpb, gw)
        return (None if gpa is None else gpa.to(points1.dtype).view(points1.shape),
                None if gpb is None else gpb.to(points2.dtype).view(points2.shape),
                None if gw is None else gw.to(weights.dtype).view(weights.shape))


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _fit(points1, points2, weights, reweight, huber_k, n_irls):
    differentiable = reweight == 0 and _wants_grad(points1, points2, weights)
    if differentiable and points1.shape[1] > ops.HFIT_SINGLE_MAX:
        # (before any device work: the streaming fit has no backward, and an H without a graph is what this refuses to return)
        raise NotImplementedError(f"the weighted least-squares fit is differentiable for N <= {ops.HFIT_SINGLE_MAX} correspondences "
                                  f"per element (HFIT_SINGLE_MAX), got N = {points1.shape[1]}: subsample, or detach the inputs")
    if not points1.is_cuda:
        # The reference's QR estimator takes tensors of any device (least_squares_H.py:142-210 has no device check; only the IRLS
        # variant asserts, :292-293 -- and so does find_homography_IRLSq_QR below).  Host tensors are copied to the HIP device,
        # fitted by the same kernel and the result handed back on the caller's device: there is no CPU solver here.  (.to() is a
        # torch op: with gradients wanted, autograd carries them back over both copies.)
        dev = torch.device("cuda")
        out = _fit(points1.to(dev), points2.to(dev), None if weights is None else weights.to(dev), reweight, huber_k, n_irls)
        return out.to(points1.device)
    if differentiable:
        if weights is not None and weights.numel() != points1.shape[0] * points1.shape[1]:
            raise AssertionError(weights.shape)
        return _WeightedLSqFit.apply(points1, points2, weights)
    return _launch(points1, points2, weights, reweight, huber_k, n_irls)


def _fit_callable(points1, points2, weights, reweighting_fn, n_iter):
    """IRLS with an arbitrary loss (least_squares_H.py:323-337): every pass is one device-side re-weighted solve
    (woft_hfit_step) that also returns the residuals A x - b of its solution on the weighted system; the user's
    callable sees them as a (1, 2N, 1) device tensor -- two consecutive rows per correspondence, the reference's
    row order -- and its result, square-rooted, re-weights the rows of the next pass."""
    B, N = points1.shape[0], points1.shape[1]
    dev = points1.device
    out = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    res = torch.empty(2 * N, dtype=torch.float32, device=dev)
    for b in range(B):
        pa, pb, w = _operands(points1, points2, weights, b)
        rew = None
        for it in range(n_iter + 1):
            ops.hfit_step(pa, pb, w, rew, it == 0, res, out[b].view(9), status[b:b + 1])
            rew = torch.sqrt(reweighting_fn(res.view(1, 2 * N, 1))).to(dtype=torch.float32, device=dev)
            rew = rew.expand(1, 2 * N, 1).reshape(-1).contiguous()
    return out


def find_homography_nonhomogeneous_QR(points1, points2, weights=None):
    """Weighted inhomogeneous DLT, h33 = 1 (least_squares_H.py:142-210).
    points (B,N,2), weights (B,N) -> (B,3,3) mapping points1 -> points2.
    Differentiable once, as the reference's is through torch.linalg.qr: with grad enabled and a points1, points2 or weights that
    requires grad, H carries a graph whose backward is one HIP launch (N <= 2048 per element; above that NotImplementedError --
    never an H without a graph).  An element whose fit fails (NaN H) gets zero gradients, not torch's NaN."""
    rec = recorder()
    if rec is not None:                  # (woft_amd.probe: the tracker is finding out what a config's estimator does)
        return rec.fit("lsq", points1, points2, weights)
    _check(points1, points2)
    return _fit(points1, points2, weights, 0, 0.0, 0)


def find_homography_IRLSq_QR(points1, points2, weights=None, reweighting_fn=IRLSq_L1, n_iter=5):
    """IRLS m-estimator (least_squares_H.py:280-346): n_iter + 1 solves, per-row re-weighting
    sqrt(reweighting_fn(A x - b)) from the weighted algebraic residual.  Losses built from IRLSq_L1 / IRLSq_Huber
    (what the reference's configs use, configs/..._wIRLSq.py:24-31) run in ONE launch; any other callable is
    driven pass by pass on device tensors (_fit_callable).  Forward only, built-in losses and callables alike: the H returned
    carries no autograd graph."""
    rec = recorder()
    if rec is not None:
        return rec.fit("irls", points1, points2, weights, reweighting_fn, n_iter)
    _check(points1, points2)
    if not points1.is_cuda:
        raise AssertionError("correspondences should be on GPU")
    try:
        kind = reweighting_fn(_Probe())
    except Exception:
        kind = None
    if isinstance(kind, tuple) and len(kind) == 3 and kind[2] == 1e-8:
        if kind[0] == "l1":
            return _fit(points1, points2, weights, 1, 0.0, n_iter)
        if kind[0] == "huber":
            return _fit(points1, points2, weights, 2, kind[1], n_iter)
    return _fit_callable(points1, points2, weights, reweighting_fn, n_iter)


def find_homography_cvransac(pts_A, pts_B, weights=None, max_iters=10000, thr=1.4142, conf=0.995, seed=0):
    """RANSAC homography (least_squares_H.py:366-396, cv2.findHomography(..., cv2.RANSAC) there), on the HIP device
    (csrc/ransac.hip; semantics and deviations in DESIGN.md, "RANSAC").  pts (B,N,2) -> (B,3,3) float64, H / H[2,2], on
    pts_A's device; numpy in, numpy out.  `weights` is accepted and ignored, as cv2 ignores it.  Every batch element is fitted
    independently with the same `seed`.  Where no model is found (no hypothesis with 4 or more inliers) that element's H is
    all NaN; the reference raises a TypeError there (None[2, 2]).  Forward only (no autograd graph), as cv2 is."""
    rec = recorder()
    if rec is not None:
        return rec.fit("ransac", pts_A, pts_B, weights, ransac=(max_iters, thr, conf))
    N = pts_A.shape[1]
    assert N >= 4, "Not enough correspodences for RANSAC"
    using_torch = isinstance(pts_A, torch.Tensor)
    a = pts_A if using_torch else torch.from_numpy(np.ascontiguousarray(pts_A))
    b = pts_B if using_torch else torch.from_numpy(np.ascontiguousarray(pts_B))
    if tuple(a.shape) != tuple(b.shape) or a.dim() != 3 or a.shape[-1] != 2:
        raise AssertionError((tuple(a.shape), tuple(b.shape)))
    dev = a.device if a.is_cuda else torch.device("cuda")      # (host inputs: fitted on the HIP device, handed back)
    B = a.shape[0]
    out = torch.empty(B, 9, dtype=torch.float32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    for k in range(B):
        pa = a[k].to(device=dev, dtype=torch.float32).contiguous()
        pb = b[k].to(device=dev, dtype=torch.float32).contiguous()
        ops.ransac(pa, pb, out[k], status[k:k + 1], max_iters=max_iters, thr=thr, conf=conf, seed=seed)
    H = out.double().view(B, 3, 3)
    H = H / H[:, 2:3, 2:3]
    if not using_torch:
        return H.cpu().numpy()
    return H.to(pts_A.device)


def find_homography_TRS(pts_A, pts_B, weights=None, max_iters=10000, thr=3.0, conf=0.999, seed=0):
    """RANSAC similarity -- translation, rotation, scale -- as a homography (least_squares_H.py:349-363,
    cv2.estimateAffinePartial2D(..., method=cv2.RANSAC, ransacReprojThreshold=3, maxIters=10000, confidence=0.999) there: its
    fixed parameters are the defaults here), on the HIP device (csrc/trs.hip; semantics and deviations in DESIGN.md, "TRS").
    pts (B,N,2) -> (B,3,3) float64 with last row (0, 0, 1), on pts_A's device; numpy in, numpy out.  `weights` is accepted and
    ignored, as the reference ignores it.  Every batch element is fitted independently with the same `seed`.  Where no model
    is found (no hypothesis with 2 or more inliers) that element's H is all NaN; the reference fails there on cv2's None.
    Forward only (no autograd graph), as cv2 is."""
    rec = recorder()
    if rec is not None:
        return rec.fit("trs", pts_A, pts_B, weights, ransac=(max_iters, thr, conf))
    N = pts_A.shape[1]
    assert N >= 2, "Not enough correspodences for a similarity"
    using_torch = isinstance(pts_A, torch.Tensor)
    a = pts_A if using_torch else torch.from_numpy(np.ascontiguousarray(pts_A))
    b = pts_B if using_torch else torch.from_numpy(np.ascontiguousarray(pts_B))
    if tuple(a.shape) != tuple(b.shape) or a.dim() != 3 or a.shape[-1] != 2:
        raise AssertionError((tuple(a.shape), tuple(b.shape)))
    dev = a.device if a.is_cuda else torch.device("cuda")      # (host inputs: fitted on the HIP device, handed back)
    B = a.shape[0]
    out = torch.empty(B, 9, dtype=torch.float32, device=dev)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    for k in range(B):
        pa = a[k].to(device=dev, dtype=torch.float32).contiguous()
        pb = b[k].to(device=dev, dtype=torch.float32).contiguous()
        ops.trs(pa, pb, out[k], status[k:k + 1], max_iters=max_iters, thr=thr, conf=conf, seed=seed)
    H = out.double().view(B, 3, 3)
    if not using_torch:
        return H.cpu().numpy()
    return H.to(pts_A.device)


def torch_proj_errors(GT_H, pts_A, pts_B):
    """L2 distance between H * pts_A and pts_B (least_squares_H.py:474-489).
    GT_H (B,3,3); pts (B,2,N) -> (B,N)."""
    rec = recorder()
    if rec is not None:
        return rec.proj(GT_H, pts_A, pts_B)
    ones = torch.ones_like(pts_A[:, :1])
    proj = torch.matmul(GT_H, torch.cat([pts_A, ones], dim=1))
    z = proj[:, 2:3]
    scale = torch.where(z.abs() > 1e-8, 1.0 / (z + 1e-8), torch.ones_like(z))
    return torch.sqrt(torch.square(scale * proj[:, :2] - pts_B).sum(dim=1))


# ---- projection-error helpers (least_squares_H.py:400-505) -----------------------------------------------------------------
# Plain torch ops on the caller's device, batched; not a hot path, no kernel.  The homogeneous conversions follow the rule
# torch_proj_errors uses above (kornia's convert_points_from_homogeneous: scale = 1 / (z + 1e-8) where |z| > 1e-8, else 1).
# They are differentiable as torch ops are.  Of the HIP estimators above, find_homography_nonhomogeneous_QR is differentiable
# too (N <= 2048 per element): a training loss built from these helpers reaches the correspondences and the weights through
# that fit.  The IRLS and RANSAC estimators are forward only: their H carries no autograd graph.
def torch_e2p(pts):
    """Euclidean -> homogeneous: (B, 2, N) -> (B, 3, N), a row of ones appended (least_squares_H.py:440-449)."""
    return torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)


def torch_p2e(homo):
    """Homogeneous -> Euclidean: (B, 3, N) -> (B, 2, N) (least_squares_H.py:452-461)."""
    z = homo[:, -1:]
    scale = torch.where(z.abs() > 1e-8, 1.0 / (z + 1e-8), torch.ones_like(z))
    return scale * homo[:, :-1]


def torch_H_proj(H, pts):
    """Points warped by homographies: H (B, 3, 3), pts (B, 2, N) -> (B, 2, N) (least_squares_H.py:464-471)."""
    return torch_p2e(torch.matmul(H, torch_e2p(pts)))


def torch_reproj_errors(GT_H, est_H, pts_A):
    """L2 distance between pts_A and inv(est_H) * GT_H * pts_A: forward by the ground truth, back by the estimate
    (least_squares_H.py:400-419; the training configs' loss_fn).  GT_H, est_H (B, 3, 3); pts_A (B, 2, N) -> (B, N).
    A torch op: gradients flow to est_H, and on through find_homography_nonhomogeneous_QR where it made est_H (N <= 2048); the
    IRLS and RANSAC estimators are forward only (see above)."""
    reproj = torch_p2e(torch.linalg.inv(est_H) @ torch.matmul(GT_H, torch_e2p(pts_A)))
    return torch.sqrt(torch.square(reproj - pts_A).sum(dim=1))


def torch_proj_diff_errors(GT_H, est_H, pts_A):
    """L2 distance between GT_H * pts_A and est_H * pts_A (least_squares_H.py:422-437).
    GT_H, est_H (B, 3, 3); pts_A (B, 2, N) -> (B, N)."""
    return torch.sqrt(torch.square(torch_H_proj(GT_H, pts_A) - torch_H_proj(est_H, pts_A)).sum(dim=1))


def reproj_errors(GT_H, est_H, pts_A, mean=True):
    """The numpy form of torch_reproj_errors for one homography pair (least_squares_H.py:492-502): GT_H, est_H (3, 3),
    pts_A (2, N); the composed homography is normalised to h33 = 1 and the division by z is plain.  -> the mean error as a
    float, or the (N,) errors when mean is False."""
    Hfb = compose_H(GT_H, np.linalg.inv(est_H))
    p = np.matmul(Hfb, np.vstack((pts_A, np.ones(pts_A.shape[1]))))
    err = np.sqrt(np.square(p[:-1] / p[-1:] - pts_A).sum(axis=0))
    return float(err.mean()) if mean else err


def compose_H(*Hs):
    """Compose homographies: compose_H(H1, ..., Hk) = normalise(Hk ... H1)
    (/root/reference/pytracking/utils/geom_utils.py:365-373)."""
    for H in Hs:
        if H is None:
            return None
    result = np.eye(3)
    for H in Hs:
        result = np.dot(H, result)
    return result / result[2, 2]
