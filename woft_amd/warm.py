"""RAFT warm start on video (raft_core/utils/utils.py:28-56): carry the 1/8-resolution flow of one frame pair to the next.

    low = provider.flow_low()                                   # after compute_flow(frame[t-1], frame[t])
    provider.compute_flow(frame[t], frame[t+1], flow_init=forward_interpolate(low))

DESIGN.md section 13 has the semantics (validity, distance, tie rule) and the deviation from the reference."""
import torch

from . import ops


def forward_interpolate(flow_low):
    """(2, hf, wf) or (1, 2, hf, wf) float device tensor -> a new fp32 tensor of the same shape: every grid cell receives the flow
    of the valid point that lands nearest to it (woft_forward_interpolate).  Device in, device out: there is no host path."""
    if not isinstance(flow_low, torch.Tensor) or not flow_low.is_cuda:
        raise TypeError("forward_interpolate takes a device tensor (the provider's flow_low())")
    shape = tuple(flow_low.shape)
    t = flow_low[0] if (flow_low.dim() == 4 and shape[0] == 1) else flow_low
    if t.dim() != 3 or t.shape[0] != 2 or not t.is_floating_point():
        raise ValueError(f"forward_interpolate takes a float (2, hf, wf) or (1, 2, hf, wf) tensor, got {shape} {flow_low.dtype}")
    return ops.forward_interpolate(t.detach().to(torch.float32).contiguous()).reshape(shape)
