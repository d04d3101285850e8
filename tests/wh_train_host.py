"""Plain-torch restatement of the weight head on explicit inputs, and the stage-wise backward formulas that the kernels of
woft_amd/csrc/wh_train.hip implement.  Checker code: any dtype, any device, no HIP.

Inputs: x5 (n_win, 5, 9, 9) the head's patches of the listed windows [4 lookup levels | mean response]; params = the eight
tensors weight_head.net.{0,2,4,6}.{weight,bias}; index (n_win,) the 1/8-resolution cell of each window; mask (hf * wf, 576)
the upsampling-mask logits, row = cell, column = k * 64 + (y & 7) * 8 + (x & 7); pts (n, 2) = (x, y) pixels of the un-padded
image; crop = (top, left) of that image inside the padded one.
"""
import torch
import torch.nn.functional as F


def x5_from_rows(corr_rows, wmean, index):
    """Device rows -> x5: corr_rows (P, >= 324) the final lookup (channel t * 4 + level at window position t), wmean (P,)."""
    li = index.long()
    x = corr_rows[li, :324].reshape(-1, 81, 4).permute(0, 2, 1).reshape(-1, 4, 9, 9)
    m = wmean[li].reshape(-1, 1, 1, 1).expand(-1, 1, 9, 9)
    return torch.cat([x, m], dim=1)


def head(x5, params):
    """-> (a1, a2, a3, wl): the three activations (n_win, 128, 9, 9) and the window logits (n_win,)."""
    w0, b0, w2, b2, w4, b4, w6, b6 = params
    a1 = F.relu(F.conv2d(x5, w0, b0, padding=1))
    a2 = F.relu(F.conv2d(a1, w2, b2, padding=1))
    a3 = F.relu(F.conv2d(a2, w4, b4, padding=1))
    wl = F.conv2d(a3, w6, b6).reshape(a3.shape[0], 81).mean(dim=1)
    return a1, a2, a3, wl


def _cells(pts, crop, hf, wf):
    X = pts[:, 0].to(torch.int64) + crop[1]
    Y = pts[:, 1].to(torch.int64) + crop[0]
    return Y >> 3, X >> 3, (Y & 7) * 8 + (X & 7)


def _coefficients(mask, hc, wc, lane, wf):
    k = torch.arange(9, device=mask.device)
    m = mask[(hc * wf + wc)[:, None], k[None, :] * 64 + lane[:, None]]
    return torch.softmax(m, dim=1)                                            # (n, 9)


def _neighbours(hc, wc, hf, wf):
    k = torch.arange(9, device=hc.device)
    ny, nx = hc[:, None] + k[None, :] // 3 - 1, wc[:, None] + k[None, :] % 3 - 1
    inside = (ny >= 0) & (ny < hf) & (nx >= 0) & (nx < wf)
    return torch.where(inside, ny * wf + nx, torch.zeros_like(ny)), inside


def upsample_at(wlow, mask, pts, hf, wf, crop, do_sigmoid=False):
    """The x8 convex upsampling of the (hf * wf,) map wlow at the pixels pts (weighted_raft.py:92-103), zero padding."""
    hc, wc, lane = _cells(pts, crop, hf, wf)
    s = _coefficients(mask, hc, wc, lane, wf)
    q, inside = _neighbours(hc, wc, hf, wf)
    v = torch.where(inside, 8 * wlow[q], torch.zeros((), dtype=wlow.dtype, device=wlow.device))
    out = (s * v).sum(dim=1) / 8
    return torch.sigmoid(out) if do_sigmoid else out


def weights_at(x5, params, index, mask, pts, hf, wf, crop, do_sigmoid=False):
    """The whole restatement: head on the listed windows -> scattered into a zero map -> upsampled at pts."""
    wl = head(x5, params)[3]
    wlow = torch.zeros(hf * wf, dtype=wl.dtype, device=wl.device).index_put((index.long(),), wl)
    return upsample_at(wlow, mask, pts, hf, wf, crop, do_sigmoid)


# ---- the stage-wise backward, as the kernels compute it --------------------------------------------------------------------
def upsample_at_bwd(g_out, wlow, mask, pts, hf, wf, crop, do_sigmoid=False):
    """woft_convex_weights_at_bwd: g_wlow (hf * wf,)."""
    hc, wc, lane = _cells(pts, crop, hf, wf)
    s = _coefficients(mask, hc, wc, lane, wf)
    q, inside = _neighbours(hc, wc, hf, wf)
    g = g_out
    if do_sigmoid:
        sg = upsample_at(wlow, mask, pts, hf, wf, crop, True)
        g = g * (sg * (1 - sg))
    contrib = torch.where(inside, (g[:, None] / 8) * (s * 8), torch.zeros((), dtype=g.dtype, device=g.device))
    return torch.zeros(hf * wf, dtype=g.dtype, device=g.device).index_add(0, q.reshape(-1), contrib.reshape(-1))


def reduce_bwd(g_wlow, index, a3, w6):
    """woft_wh_reduce_bwd: (g_a3, g_w6, g_b6)."""
    gl = g_wlow[index.long()]
    g = gl / 81
    g_a3 = g[:, None, None, None] * w6.reshape(1, -1, 1, 1) * (a3 > 0)
    g_w6 = (g[:, None, None, None] * a3).sum(dim=(0, 2, 3)).reshape(w6.shape)
    return g_a3, g_w6, gl.sum().reshape(1)


def layer_wgrad(gy, x):
    """woft_wh_wgrad: gw[co][ci][ky][kx] = sum_{p,t} gy[p][co][t] * x[p][ci][t + k] (zero outside the window), gb = sum gy."""
    xp = F.pad(x, (1, 1, 1, 1))
    gw = torch.stack([torch.stack([torch.einsum("pcyx,pdyx->cd", gy, xp[:, :, ky:ky + 9, kx:kx + 9]) for kx in range(3)], dim=-1)
                      for ky in range(3)], dim=-2)
    return gw, gy.sum(dim=(0, 2, 3))


def layer_dgrad(gy, w, x):
    """woft_wh_train_conv with the transposed, flipped filter and the gate x > 0."""
    return F.conv2d(gy, w.flip(2, 3).transpose(0, 1), padding=1) * (x > 0)


def backward(x5, params, index, mask, pts, hf, wf, crop, g_out, do_sigmoid=False):
    """All eight parameter gradients of sum(weights_at(...) * g_out), stage by stage."""
    w0, b0, w2, b2, w4, b4, w6, b6 = params
    a1, a2, a3, wl = head(x5, params)
    wlow = torch.zeros(hf * wf, dtype=wl.dtype, device=wl.device).index_put((index.long(),), wl)
    g_wlow = upsample_at_bwd(g_out, wlow, mask, pts, hf, wf, crop, do_sigmoid)
    g_a3, g_w6, g_b6 = reduce_bwd(g_wlow, index, a3, w6)
    g_w4, g_b4 = layer_wgrad(g_a3, a2)
    g_a2 = layer_dgrad(g_a3, w4, a2)
    g_w2, g_b2 = layer_wgrad(g_a2, a1)
    g_a1 = layer_dgrad(g_a2, w2, a1)
    g_w0, g_b0 = layer_wgrad(g_a1, x5)
    return [g_w0, g_b0, g_w2, g_b2, g_w4, g_b4, g_w6, g_b6]


def autograd(x5, params, index, mask, pts, hf, wf, crop, g_out, do_sigmoid=False, dtype=torch.float64):
    """The same gradients by torch autograd of the whole restatement in `dtype` -> (values, grads)."""
    c = lambda t: t.detach().to(dtype)
    ps = [c(p).requires_grad_(True) for p in params]
    out = weights_at(c(x5), ps, index, c(mask), pts, hf, wf, crop, do_sigmoid)
    out.backward(c(g_out))
    return out.detach(), [p.grad for p in ps]


def rel_err(g, g64):
    """Section 15's convention: max |g - g64| / max |g64|."""
    g64 = g64.detach().double().cpu()
    return float((g.detach().double().cpu() - g64).abs().max() / g64.abs().max())


def random_params(gen, gain=1.0):
    """Seeded head parameters with activations of order one through all layers (He-like scaling)."""
    r = lambda *s: torch.randn(*s, generator=gen)
    return [r(128, 5, 3, 3) * gain * (2.0 / 45) ** 0.5, r(128) * 0.1, r(128, 128, 3, 3) * gain * (2.0 / 1152) ** 0.5, r(128) * 0.1,
            r(128, 128, 3, 3) * gain * (2.0 / 1152) ** 0.5, r(128) * 0.1, r(1, 128, 1, 1) * (1.0 / 128) ** 0.5, r(1) * 0.1]
