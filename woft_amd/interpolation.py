"""Using one flow together with another: the counterpart of the reference's pytracking/utils/interpolation.py
(bilinear_interpolate_torch, flow_warp_coords, chain_flow) plus the forward-backward consistency check, on the HIP kernels of
csrc/flow_chain.hip.  DESIGN.md section 16.

    flow_ac = chain_flow(flow_ab, flow_bc)
    err, ok = fb_consistency(flow_ab, flow_ba)

Device tensors go to the kernels as they are.  Host tensors are copied to the device and the result is handed back on the
caller's device (the precedent of find_homography_nonhomogeneous_QR): there is no CPU implementation.  Inputs that are not fp32
are computed in fp32 and the result is cast back to the input's dtype.  Forward only: no autograd graph.

`FlowInterpolator` and `interp_flow` of the reference (scipy on host arrays) are not provided.
"""
import torch

from . import ops


def _dev32(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: a torch tensor is expected, got {type(t).__name__}")
    if not (t.is_floating_point()):
        raise TypeError(f"{what}: a floating-point tensor is expected, got {t.dtype}")
    return t.detach().to(device="cuda", dtype=torch.float32).contiguous()


def _back(out, like):
    return out.to(device=like.device, dtype=like.dtype)


def bilinear_interpolate_torch(data, x, y):
    """Bilinear interpolation of a (C, H, W) tensor at N points (interpolation.py:92-133), the reference's fp32 arithmetic bit
    for bit -- including its edge behaviour: a point on or beyond the last row / column, or left of / above the first, samples 0.

    args:
        data: (C, H, W) tensor with data to be interpolated
        x: (N, ) tensor with x coordinates into data
        y: (N, ) tensor with y coordinates into data
    returns:
        interp: (C, N) tensor with values interpolated from data (data's device and dtype; computed in fp32)
    """
    if data.dim() != 3 or x.dim() != 1 or y.shape != x.shape:
        raise ValueError(f"bilinear_interpolate_torch takes (C, H, W), (N,), (N,); got {tuple(data.shape)}, {tuple(x.shape)}, "
                         f"{tuple(y.shape)}")
    out = ops.sample_bilinear(_dev32(data, "data"), _dev32(x, "x"), _dev32(y, "y"))
    return _back(out, data)


def flow_warp_coords(coords_A, flow_AB):
    """Warp (non-integer) coordinates coords_A using optical flow (interpolation.py:74-89).

    args:
        coords_A: (2, N) tensor with x, y coordinates
        flow_AB: (2, H, W) tensor with optical flow
    returns:
        coords_B: (2, N) tensor with x, y coordinates (coords_A's device and dtype; computed in fp32)
    """
    if coords_A.dim() != 2 or coords_A.shape[0] != 2 or flow_AB.dim() != 3 or flow_AB.shape[0] != 2:
        raise ValueError(f"flow_warp_coords takes (2, N) and (2, H, W); got {tuple(coords_A.shape)}, {tuple(flow_AB.shape)}")
    c = _dev32(coords_A, "coords_A")
    sampled = ops.sample_bilinear(_dev32(flow_AB, "flow_AB"), c[0].contiguous(), c[1].contiguous())
    return _back(c + sampled, coords_A)


def _flows(a, b, names):
    if a.shape != b.shape or a.dim() not in (3, 4) or a.shape[-3] != 2:
        raise ValueError(f"{names[0]} and {names[1]} must both be (2, H, W) or (B, 2, H, W); got {tuple(a.shape)}, {tuple(b.shape)}")
    a32, b32 = _dev32(a, names[0]), _dev32(b, names[1])
    return (a32[None], b32[None], False) if a.dim() == 3 else (a32, b32, True)


def chain_flow(flow_AB, flow_BC):
    """Chain flow by bilinear interpolation (interpolation.py:9-23, finished): flow_AC = flow_AB + flow_BC sampled at
    pixel + flow_AB, with the edge-exact sampler (the last row / column return the data there).  A pixel whose flow_AB leaves
    the frame gets NaN in both planes.  (B, 2, H, W) or (2, H, W); `flow_AB is None` returns flow_BC, as in the reference.
    Computed in fp32; the result has flow_AB's device and dtype."""
    if flow_AB is None:
        return flow_BC
    a, b, batched = _flows(flow_AB, flow_BC, ("flow_AB", "flow_BC"))
    out = torch.empty_like(a)
    for i in range(a.shape[0]):
        ops.flow_chain(a[i], b[i], out[i])
    return _back(out if batched else out[0], flow_AB)


def fb_consistency(flow_AB, flow_BA, alpha=0.01, beta=0.5):
    """Forward-backward consistency of two flows -> (err, ok), each (1, H, W) or (B, 1, H, W) on flow_AB's device, in its dtype.
    With b = flow_BA sampled at pixel + flow_AB: err = |flow_AB + b| (pixels), ok = 1.0 where that point is inside the frame and
    err^2 <= alpha * (|flow_AB|^2 + |b|^2) + beta, else 0.0.  A pixel whose flow leaves the frame: err = +inf, ok = 0.
    alpha, beta: finite floats >= 0.  Computed in fp32."""
    alpha, beta = float(alpha), float(beta)
    if not (0.0 <= alpha < float("inf")) or not (0.0 <= beta < float("inf")):
        raise ValueError(f"fb_consistency: alpha and beta must be finite and >= 0, got {alpha!r}, {beta!r}")
    a, b, batched = _flows(flow_AB, flow_BA, ("flow_AB", "flow_BA"))
    n, _, h, w = a.shape
    err, ok = torch.empty((n, 1, h, w), device=a.device), torch.empty((n, 1, h, w), device=a.device)
    for i in range(n):
        ops.flow_fb(a[i], b[i], alpha, beta, err[i, 0], ok[i, 0])
    if not batched:
        err, ok = err[0], ok[0]
    return _back(err, flow_AB), _back(ok, flow_AB)
