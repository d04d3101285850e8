"""Training of the visibility MaskHead on HIP (DESIGN.md sections 21, 22): the autograd nodes behind RAFTWrapper.visibility_at()
and RAFTWrapper.visibility_map().

The exact analogue of wh_train.py for the reference's second head (weighted_raft.py:387-422, raft_type 'weighted_masked'): a frozen
RAFT and a trainable MaskHead -- 3x3 convs with a ReLU after each over the whole 1/8-resolution map of [fmap1 | warped fmap2]
(weighted_raft.py:295-304), a closing 1x1 conv, the x8 convex upsampling the weights share (weighted_raft.py:305-308).  This node
carries the gradient from the visibility at a list of pixels (or, VisibilityMap, at every pixel) into the head's parameters; it stops at the head's inputs (fmap1, the
warped fmap2, the upsampling mask, the points): RAFT stays frozen.
"""
from collections import OrderedDict

import torch

from . import ops

MAX_C = 128


def names(n_layers):
    """State-dict names of a head of n_layers 3x3 layers and its closing conv: mask_head.net.{0,2,...,2 n_layers}.{weight,bias}."""
    return tuple(f"mask_head.net.{2 * k}.{s}" for k in range(n_layers + 1) for s in ("weight", "bias"))


def refusal(shapes):
    """Why the training kernels do not cover a head whose mask_head.net.*.weight shapes are `shapes`, or None if they do: every
    layer before the closing 1x1 conv is (C, cin, 3, 3) with C a multiple of 32 and at most 128."""
    for co, _, kh, kw in shapes[:-1]:
        if (kh, kw) != (3, 3):
            return f"a mask_head_structure layer of kernel size {kh} (only 3)"
        if co % 32 != 0 or co > MAX_C:
            return f"a mask_head_structure layer of {co} channels (only multiples of 32 up to {MAX_C})"
    return None


def make_parameters(state_dict, shapes):
    """The head's tensors of a reference-format state dict -> OrderedDict of fp32 device Parameters under the same names."""
    why = refusal(shapes)
    if why:
        raise NotImplementedError(f"training of the mask head is not provided for {why}")
    out = OrderedDict()
    for name in names(len(shapes) - 1):
        t = state_dict[name].detach().to(device="cuda", dtype=torch.float32).clone().contiguous()
        out[name] = torch.nn.Parameter(t, requires_grad=True)
    return out


def head_forward(x0, x1, hf, wf, params, acts, out):
    """The head up to (not including) its closing bias on the hf x wf map [x0 | x1] (maps: (rows >= hf * wf, channel stride) fp32;
    x1 None: x0 alone): params = (w0, b0, ..., w_{L-1}, b_{L-1}, w_last) in state-dict shapes, acts = L maps that receive the
    activations, out[:hf * wf] = <w_last, act_L>.  Exact fp32."""
    P = hf * wf
    x = (x0, x1)
    for k, a in enumerate(acts):
        w, b = params[2 * k], params[2 * k + 1]
        wt = w.permute(2, 3, 1, 0).reshape(9, w.shape[1], w.shape[0]).contiguous()          # forward weights [tap][ci][co]
        ops.mh_train_conv(x[0], x[1], wt, hf, wf, a, bias=b.contiguous())
        x = (a, None)
    last = acts[-1]
    w_last = torch.zeros(last.shape[1], dtype=torch.float32, device=last.device)             # (woft_wh_reduce walks whole rows)
    w_last[:params[-1].numel()] = params[-1].reshape(-1)
    ops.wh_reduce(ops.Act(last, 1, hf, wf, params[-1].numel()), 1, w_last, 0.0, P, out)


def head_backward(x0, x1, hf, wf, params, acts, g_low, gbufs, ws, ws64, grads):
    """Backward of head_forward (+ the closing bias): g_low (hf * wf,) = the gradient of the 1/8-resolution logits; params =
    (w_1, ..., w_{L-1}, w_last), the weights the data gradients read, as the forward read them; gbufs = two maps as wide as the
    widest layer; ws, ws64 = the partial-sum workspaces of woft_mh_wgrad / woft_mh_reduce_bwd; grads = the 2 L + 2 outputs in
    state-dict order."""
    P, L = hf * wf, len(acts)
    gA, gB = gbufs
    w_last = params[-1].reshape(-1).contiguous()
    ops.mh_reduce_bwd(acts[-1], w_last.numel(), w_last, g_low, P, gA, ws64, grads[2 * L].view(-1), grads[2 * L + 1])
    for k in range(L - 1, -1, -1):
        below = (acts[k - 1], None) if k > 0 else (x0, x1)
        ops.mh_wgrad(gA, below[0], below[1], hf, wf, ws, grads[2 * k], grads[2 * k + 1])
        if k > 0:                                                     # (the first layer's inputs are frozen: no data gradient)
            w = params[k - 1]
            flipped = w.flip(2, 3).permute(2, 3, 0, 1).reshape(9, w.shape[0], w.shape[1]).contiguous()      # [tap][co][ci]
            ops.mh_train_conv(gA, None, flipped, hf, wf, gB, gate=acts[k - 1])
            gA, gB = gB, gA


class VisibilityAt(torch.autograd.Function):
    """vis = plan.mh_train_forward(...) with a backward into the head's parameters (plan.mh_train_backward).  Once differentiable,
    like wh_train.WeightsAt; pts, count and everything the frozen network computed get no gradient."""

    @staticmethod
    def forward(ctx, plan, pts, count, n_max, crop, do_sigmoid, *params):
        vsel, state = plan.mh_train_forward(params, pts, count, n_max, crop, do_sigmoid)
        ctx.plan, ctx.state = plan, state
        return vsel

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        grads = ctx.plan.mh_train_backward(ctx.state, grad_output.to(torch.float32).contiguous())
        need = ctx.needs_input_grad[6:]
        return (None,) * 6 + tuple(g if n else None for g, n in zip(grads, need))


def visibility_at(plan, params, pts, count, n_max, crop, do_sigmoid):
    params = tuple(params)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return VisibilityAt.apply(plan, pts, count, n_max, crop, bool(do_sigmoid), *params)
    return plan.mh_train_forward(params, pts, count, n_max, crop, do_sigmoid)[0]


class VisibilityMap(torch.autograd.Function):
    """The dense form: map = plan.mh_dense_forward(...), the visibility at every pixel of the un-padded
    image, with a backward into the head's parameters (plan.mh_dense_backward: the dense adjoint of the convex upsampling, then
    the same head backward).  Once differentiable; nothing but the parameters gets a gradient."""

    @staticmethod
    def forward(ctx, plan, crop, h, w, do_sigmoid, *params):
        out, state = plan.mh_dense_forward(params, crop, h, w, do_sigmoid)
        ctx.plan, ctx.state = plan, state
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        grads = ctx.plan.mh_dense_backward(ctx.state, grad_output.to(torch.float32).contiguous())
        need = ctx.needs_input_grad[5:]
        return (None,) * 5 + tuple(g if n else None for g, n in zip(grads, need))


def visibility_map(plan, params, crop, h, w, do_sigmoid):
    params = tuple(params)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return VisibilityMap.apply(plan, crop, h, w, bool(do_sigmoid), *params)
    return plan.mh_dense_forward(params, crop, h, w, do_sigmoid)[0]
