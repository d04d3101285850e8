"""Training of the flow-reliability weight head on HIP: the autograd node behind
RAFTWrapper.weights_at().

The reference trains exactly this (optical_flow/training_configs/*.py with train_flow = False): a frozen RAFT and a trainable
WeightHead (weighted_raft.py:318-384), through re-projection loss -> weighted homography fit -> weights -> head.  The fit's
backward is homography._WeightedLSqFit; this node carries the gradient from the weights into the head's parameters.  The gradient
stops at the head's inputs (final lookup, mean response, upsampling mask, the points): RAFT stays frozen.
"""
from collections import OrderedDict

import torch

from . import ops

NAMES = tuple(f"weight_head.net.{i}.{s}" for i in (0, 2, 4, 6) for s in ("weight", "bias"))
SHAPES = ((128, 5, 3, 3), (128,), (128, 128, 3, 3), (128,), (128, 128, 3, 3), (128,), (1, 128, 1, 1), (1,))


def make_parameters(state_dict):
    """The head's tensors of a reference-format state dict -> OrderedDict of fp32 device Parameters under the same names."""
    out = OrderedDict()
    for name, shape in zip(NAMES, SHAPES):
        t = state_dict[name].detach().to(device="cuda", dtype=torch.float32).clone().contiguous()
        if tuple(t.shape) != shape:
            raise NotImplementedError(f"weights_at() trains the standard head only: {name} is {tuple(t.shape)}, not {shape}")
        out[name] = torch.nn.Parameter(t, requires_grad=True)
    return out


def head_forward(x8, n_win, params, acts, out):
    """The head up to (not including) its closing bias on n_win windows: x8 (>= n_win, 81, 8) woft_wh_pack rows, params =
    (w0, b0, w2, b2, w4, b4, w6) in state-dict shapes, acts = three (>= n_win, 81, 128) buffers that receive the activations,
    out[:n_win] = mean over the window of <w6, act3>.  Exact fp32."""
    w0, b0, w2, b2, w4, b4, w6 = params
    # forward weights [tap][ci][co] (the first layer's 5 input channels padded to the 8 of its rows)
    wt0 = torch.zeros(9, 8, 128, dtype=torch.float32, device=x8.device)
    wt0[:, :5] = w0.permute(2, 3, 1, 0).reshape(9, 5, 128)
    wt2, wt4 = (w.permute(2, 3, 1, 0).reshape(9, 128, 128).contiguous() for w in (w2, w4))
    a1, a2, a3 = acts
    ops.wh_train_conv(x8, 8, wt0, n_win, a1, bias=b0.contiguous())
    ops.wh_train_conv(a1, 128, wt2, n_win, a2, bias=b2.contiguous())
    ops.wh_train_conv(a2, 128, wt4, n_win, a3, bias=b4.contiguous())
    ops.wh_reduce(ops.Act(a3.view(-1, 128)[:n_win * 81], n_win, 9, 9, 128), 81, w6.reshape(-1).contiguous(), 0.0, n_win, out)


def head_backward(x8, n_win, params, acts, g_wlow, index, gbufs, ws, ws64, grads):
    """Backward of head_forward (+ the closing bias): g_wlow = the gradient of the 1/8-resolution logits, read at index[p] for
    window p (index None: at p); params = (w2, w4, w6) as the forward read them; gbufs = two (>= n_win, 81, 128) buffers; ws,
    ws64 = the partial-sum workspaces of woft_wh_wgrad / woft_wh_reduce_bwd; grads = the eight outputs in state-dict order."""
    w2, w4, w6 = params
    a1, a2, a3 = acts
    gA, gB = gbufs
    gw0, gb0, gw2, gb2, gw4, gb4, gw6, gb6 = grads
    ops.wh_reduce_bwd(a3, w6.reshape(-1).contiguous(), g_wlow, index, n_win, gA, ws64, gw6.view(-1), gb6)
    flipped = lambda w: w.flip(2, 3).permute(2, 3, 0, 1).reshape(9, 128, 128).contiguous()    # data gradient: [tap][co][ci]
    ops.wh_wgrad(gA, a2, 128, n_win, ws, gw4, gb4)
    ops.wh_train_conv(gA, 128, flipped(w4), n_win, gB, gate=a2)
    ops.wh_wgrad(gB, a1, 128, n_win, ws, gw2, gb2)
    ops.wh_train_conv(gB, 128, flipped(w2), n_win, gA, gate=a1)
    ops.wh_wgrad(gA, x8, 8, n_win, ws, gw0, gb0)


class WeightsAt(torch.autograd.Function):
    """weights = plan.wh_train_forward(...) with a backward into the eight head parameters (plan.wh_train_backward).  Once
    differentiable, like homography._WeightedLSqFit; pts, count and everything the frozen network computed get no gradient."""

    @staticmethod
    def forward(ctx, plan, pts, count, n_max, pad, do_sigmoid, *params):
        wsel, state = plan.wh_train_forward(params, pts, count, n_max, pad, pad, do_sigmoid)
        ctx.plan, ctx.state = plan, state
        return wsel

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        grads = ctx.plan.wh_train_backward(ctx.state, grad_output.to(torch.float32).contiguous())
        need = ctx.needs_input_grad[6:]
        return (None,) * 6 + tuple(g if n else None for g, n in zip(grads, need))


def weights_at(plan, params, pts, count, n_max, pad, do_sigmoid):
    params = tuple(params)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return WeightsAt.apply(plan, pts, count, n_max, pad, bool(do_sigmoid), *params)
    return plan.wh_train_forward(params, pts, count, n_max, pad, pad, do_sigmoid)[0]
