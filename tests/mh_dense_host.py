"""Plain-torch restatement of the dense visibility map (weighted_raft.py:92-103, 305-308) on explicit inputs: what
woft_convex_upsample_bwd and RAFTWrapper.visibility_map are checked against.  Checker code: any dtype, any
device, no HIP.

Inputs as in tests/mh_train_host.py: low (hf * wf,) the 1/8-resolution logits; mask (rows >= hf * wf, columns >= 576) the
upsampling-mask logits, row = cell, column = k * 64 + (y & 7) * 8 + (x & 7); crop = (top, left) of the (h, w) un-padded image
inside the padded (8 hf, 8 wf) one.
"""
import torch
import torch.nn.functional as F

from mh_train_host import head, rel_err  # noqa: F401


def upsample_dense(low, mask, hf, wf, crop, h, w, do_sigmoid=False):
    """The x8 convex upsampling of the whole map as the reference writes it (unfold of 8 * low, softmax over the nine taps), then
    the / 8 the weights and the visibility take, the crop and the optional sigmoid -> (h, w)."""
    m = mask[:hf * wf, :576].t().reshape(1, 1, 9, 8, 8, hf, wf)
    m = torch.softmax(m, dim=2)
    up = F.unfold(8 * low.reshape(1, 1, hf, wf), [3, 3], padding=1)
    up = up.view(1, 1, 9, 1, 1, hf, wf)
    up = torch.sum(m * up, dim=2)
    up = up.permute(0, 1, 4, 2, 5, 3).reshape(8 * hf, 8 * wf) / 8
    out = up[crop[0]:crop[0] + h, crop[1]:crop[1] + w]
    return torch.sigmoid(out) if do_sigmoid else out


def low_grad(low, mask, hf, wf, crop, h, w, g_up, do_sigmoid=False, dtype=torch.float64):
    """The gradient of sum(upsample_dense(...) * g_up) with respect to low by torch autograd in `dtype` -> (hf * wf,)."""
    lo = low.detach().to(dtype).requires_grad_(True)
    out = upsample_dense(lo, mask.detach().to(dtype), hf, wf, crop, h, w, do_sigmoid)
    out.backward(g_up.detach().to(dtype).reshape(h, w))
    return lo.grad


def visibility_map(x, params, mask, hf, wf, crop, h, w, do_sigmoid=False):
    """The whole restatement: head over the map -> logits -> upsampled everywhere."""
    return upsample_dense(head(x, params)[1], mask, hf, wf, crop, h, w, do_sigmoid)


def autograd_dense(x, params, mask, hf, wf, crop, h, w, g_out, do_sigmoid=False, dtype=torch.float64):
    """Values and all parameter gradients of sum(map * g_out) by torch autograd in `dtype` -> (values (h, w), grads)."""
    c = lambda t: t.detach().to(dtype)
    ps = [c(p).requires_grad_(True) for p in params]
    out = visibility_map(c(x), ps, c(mask), hf, wf, crop, h, w, do_sigmoid)
    out.backward(c(g_out).reshape(h, w))
    return out.detach(), [p.grad for p in ps]
