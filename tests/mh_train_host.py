"""Plain-torch restatement of the MaskHead (weighted_raft.py:295-309, 387-422) on explicit inputs: what the kernels of
woft_amd/csrc/mh_train.hip are checked against.  Checker code: any dtype, any device, no HIP.

Inputs: x (1, cin, hf, wf) the head's input map [fmap1 | warped fmap2]; params = the tensors mask_head.net.{0,2,...}.{weight,bias}
in state-dict order (3x3 layers, then the closing 1x1 conv); mask (hf * wf, 576) the upsampling-mask logits, row = cell, column =
k * 64 + (y & 7) * 8 + (x & 7); pts (n, 2) = (x, y) pixels of the un-padded image; crop = (top, left) of that image inside the
padded one.
"""
import torch
import torch.nn.functional as F

from wh_train_host import rel_err, upsample_at  # noqa: F401  (the convex upsampling at points is the weights' own)


def head(x, params):
    """-> (acts, low): the activations (1, C, hf, wf) of the 3x3 layers and the 1/8-resolution logits (hf * wf,)."""
    acts = []
    for k in range(len(params) // 2 - 1):
        x = F.relu(F.conv2d(x, params[2 * k], params[2 * k + 1], padding=1))
        acts.append(x)
    return acts, F.conv2d(x, params[-2], params[-1]).reshape(-1)


def visibility_at(x, params, mask, pts, hf, wf, crop, do_sigmoid=False):
    """The whole restatement: head over the map -> logits -> upsampled at pts."""
    return upsample_at(head(x, params)[1], mask, pts, hf, wf, crop, do_sigmoid)


def head_autograd(x, params, g_low, dtype=torch.float64):
    """Logits and all parameter gradients of sum(low * g_low) by torch autograd in `dtype` -> (low, grads, acts)."""
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    acts, low = head(x.detach().to(dtype), ps)
    (low * g_low.to(dtype)).sum().backward()
    return low.detach(), [p.grad for p in ps], [a.detach() for a in acts]


def autograd(x, params, mask, pts, hf, wf, crop, g_out, do_sigmoid=False, dtype=torch.float64):
    """Values and all parameter gradients of sum(visibility_at(...) * g_out) by torch autograd in `dtype` -> (values, grads)."""
    c = lambda t: t.detach().to(dtype)
    ps = [c(p).requires_grad_(True) for p in params]
    out = visibility_at(c(x), ps, c(mask), pts, hf, wf, crop, do_sigmoid)
    out.backward(c(g_out))
    return out.detach(), [p.grad for p in ps]


def random_params(gen, cin, channels):
    """Seeded head parameters (3x3 layers of `channels` outputs on cin inputs, then the closing conv) with activations of order
    one through all layers (He-like scaling)."""
    r = lambda *s: torch.randn(*s, generator=gen)
    out = []
    for c in channels:
        out += [r(c, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5, r(c) * 0.1]
        cin = c
    return out + [r(1, cin, 1, 1) * (1.0 / cin) ** 0.5, r(1) * 0.1]
