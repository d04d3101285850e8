"""Thin Python layer over the C ABI: tensor bookkeeping, weight packing, one function per kernel.

All tensors are torch CUDA (=HIP) tensors; the library enqueues on torch's current stream.
Activations are NHWC fp32: a tensor of shape (n_pix, channel_stride) (pixels of all images
flattened) -- `Act` carries the geometry.
"""
import ctypes as C
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, conv_select
from ._lib import ConvParams, LookupBandParams, LookupOtfParams, LookupParams, check, ptr, stream_ptr
from .conv_select import KERNELS, PRECISION, Kernel, pair_ok  # noqa: F401  (PRECISION, pair_ok: part of this module's interface)

DEV = "cuda"


def _round_up(x, m):
    return (x + m - 1) // m * m


@dataclass
class Act:
    """NHWC activation: t is (n_img*h*w, cs) fp32 contiguous; `c` valid channels."""
    t: torch.Tensor
    n: int
    h: int
    w: int
    c: int

    @property
    def cs(self):
        return self.t.shape[1]

    @property
    def n_pix(self):
        return self.n * self.h * self.w

    def nchw(self):
        """(n, c, h, w) copy -- test / boundary helper."""
        return self.t[:, :self.c].reshape(self.n, self.h, self.w, self.c).permute(0, 3, 1, 2).contiguous()


def _rows(n_pix, cs, zero):
    return (torch.zeros if zero else torch.empty)(n_pix, cs, dtype=torch.float32, device=DEV)


def act_from_nchw(x, cs=None):
    n, c, h, w = x.shape
    cs = cs or _round_up(c, 4)
    t = _rows(n * h * w, cs, True)
    t[:, :c] = x.to(DEV).permute(0, 2, 3, 1).reshape(n * h * w, c)
    return Act(t, n, h, w, c)


def new_act(n, h, w, c, cs=None, zero=False):
    cs = cs or _round_up(c, 4)
    return Act(_rows(n * h * w, cs, zero), n, h, w, c)


# ------------------------------------------------------------------------------------------
# weight packing
# ------------------------------------------------------------------------------------------
@dataclass
class PackedConv:
    wgt: torch.Tensor        # (cout_pad, taps*cin_pad) fp32 on device
    bias: torch.Tensor       # (cout_pad,)
    cout: int
    cout_pad: int
    cin_pad: int
    taps_y: int
    taps_x: int
    pad_y: int
    pad_x: int
    stride: int
    flat: int
    flat_cs: int = 0
    kh: int = 0              # real kernel size (flat packing folds kw into the K chunk)
    kw: int = 0
    wgt_hi: torch.Tensor = None   # bf16 split of wgt: hi = bf16(w), lo = bf16(w - hi)
    wgt_lo: torch.Tensor = None
    _frag: dict = None            # planes -> weights in MFMA-fragment order (woft_conv_params.wgt_frag), built on demand
    _f16: torch.Tensor = None     # fp16(w) in a bf16-typed container (precision "fp16"), built on demand

    def wgt_f16(self):
        if self._f16 is None:
            w = self.wgt.detach().cpu()
            if float(w.abs().max()) >= 65504.0:
                raise ValueError("precision 'fp16': a weight exceeds the fp16 range")
            self._f16 = w.to(torch.float16).view(torch.bfloat16).to(self.wgt.device)
        return self._f16

    def frag(self, planes, f16=False):
        """[cout_pad/32 bands][chunks][taps][planes][2 k halves][64 lanes][8] bf16 (see woft_conv_params.wgt_frag);
        f16: one plane of fp16 values in the same 16-bit containers (precision "fp16")."""
        if self._frag is None:
            self._frag = {}
        key = "f16" if f16 else planes
        if key not in self._frag:
            taps, nchunk = self.taps_y * self.taps_x, self.cin_pad // 32
            w = self.wgt.detach().cpu().reshape(self.cout_pad // 32, 32, taps, nchunk, 2, 2, 8)
            w = w.permute(0, 3, 2, 4, 5, 1, 6).contiguous()        # band, chunk, tap, k half, lane half, row, e
            if f16:
                pl = [w.to(torch.float16).view(torch.bfloat16)]
            else:
                hi = w.to(torch.bfloat16)
                pl = [hi] + ([(w - hi.float()).to(torch.bfloat16)] if planes == 2 else [])
            self._frag[key] = torch.stack(pl, dim=3).contiguous().to(self.wgt.device)
        return self._frag[key]

    def frag_mx(self):
        """fp8 fragments of the weights for precision "f16mx8" (woft_conv_params.wgt_mx): per 32-column band, 32-channel chunk, tap
        pair and term (0: w, 1: w - fp16(w)) -- 64 lanes x 32 bytes e4m3 (lane L: column L % 32; bytes 0-15 = channels 16 (L // 32)
        .. + 15 at the pair's first tap, bytes 16-31 at its second tap; an odd last tap pairs with zeros), then 64 int32 scales: lane
        half 0 carries the E8M0 scale of the (column, first tap, chunk) block, lane half 1 that of the second tap's block.  A block's
        scale puts its largest magnitude into [128, 256) (e4m3 holds up to 448)."""
        if self._frag is None:
            self._frag = {}
        if "mx" not in self._frag:
            taps, nchunk = self.taps_y * self.taps_x, self.cin_pad // 32
            npair = (taps + 1) // 2
            w = self.wgt.detach().cpu().reshape(self.cout_pad, taps, nchunk, 32)
            if float(w.abs().max()) >= 65504.0:
                raise ValueError("precision 'f16mx8': a weight exceeds the fp16 range")
            lw = w - w.to(torch.float16).float()
            bands = self.cout_pad // 32
            out = torch.zeros(bands, nchunk, npair, 2, 64 * 32 + 64 * 4, dtype=torch.uint8)
            for t, x in enumerate((w, lw)):
                amax = x.abs().amax(dim=3)                                            # [cout_pad][taps][nchunk]
                e = torch.floor(torch.log2(torch.clamp(amax, min=1e-38)))
                sc = torch.where(amax > 0, e - 7 + 127, torch.full_like(e, 127.0)).clamp(0, 254)   # E8M0 byte
                q = (x / torch.exp2(sc - 127)[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)    # [cout_pad][taps][nchunk][32]
                if taps % 2:                                                          # zero weights (and unit scale) behind an odd last tap
                    q = torch.cat([q, torch.zeros_like(q[:, :1])], 1)
                    sc = torch.cat([sc, torch.full_like(sc[:, :1], 127.0)], 1)
                q = q.reshape(bands, 32, npair, 2, nchunk, 2, 16)                     # band, col, pair, tap-in-pair, chunk, hh, 16 channels
                data = q.permute(0, 4, 2, 5, 1, 3, 6).reshape(bands, nchunk, npair, 64 * 32)    # lane = 32 hh + col; [tap0 16 B | tap1 16 B]
                scl = sc.reshape(bands, 32, npair, 2, nchunk).permute(0, 4, 2, 3, 1).reshape(bands, nchunk, npair, 64)   # lane = 32 tap-in-pair + col
                scl4 = torch.zeros(bands, nchunk, npair, 64, 4, dtype=torch.uint8)
                scl4[..., 0] = scl.to(torch.uint8)
                out[:, :, :, t, :64 * 32] = data
                out[:, :, :, t, 64 * 32:] = scl4.reshape(bands, nchunk, npair, 256)
            self._frag["mx"] = out.contiguous().to(self.wgt.device)
        return self._frag["mx"]

    def __post_init__(self):
        if self.wgt is not None and self.wgt_hi is None and self.wgt.dtype == torch.float32:
            w = self.wgt.detach().cpu()
            hi = w.to(torch.bfloat16)
            self.wgt_hi = hi.to(self.wgt.device)
            self.wgt_lo = (w - hi.float()).to(torch.bfloat16).to(self.wgt.device)

    def out_hw(self, h, w):
        kh, kw = (self.kh or self.taps_y), (self.kw or self.taps_x)
        return (h + 2 * self.pad_y - kh) // self.stride + 1, (w + 2 * self.pad_x - kw) // self.stride + 1


def pack_conv(weight, bias, stride=1, padding=None, cin_layout=None, flat_cs=0, scale=1.0):
    """OIHW conv weight -> [cout_pad][taps][cin_pad] (K contiguous).

    cin_layout: list of (src_begin, src_end, dst_begin) channel ranges mapping the reference's
                input-channel order onto the (padded) channel order of our input buffers;
                default = identity.
    flat_cs:    >0 -> "flat" packing for tiny Cin: the K chunk of tap ky is kw pixels x flat_cs
                channels laid out as the NHWC row itself (k = kx*flat_cs + c), padded to 32.
    """
    weight = weight.detach().float().cpu() * scale
    cout, cin, kh, kw = weight.shape
    if padding is None:
        padding = (kh // 2, kw // 2)
    if isinstance(padding, int):
        padding = (padding, padding)
    cout_pad = _round_up(cout, 64)
    if cout_pad > 64:
        cout_pad = _round_up(cout, 128)
    b = torch.zeros(cout_pad)
    if bias is not None:
        b[:cout] = bias.detach().float().cpu() * scale
    if flat_cs:
        assert kw * flat_cs <= 32 and cin <= flat_cs
        wp = torch.zeros(cout_pad, kh, 32)
        for kx in range(kw):
            wp[:cout, :, kx * flat_cs:kx * flat_cs + cin] = weight[:, :, :, kx].permute(0, 2, 1)
        return PackedConv(wp.reshape(cout_pad, kh * 32).contiguous().to(DEV), b.to(DEV), cout, cout_pad, 32,
                          kh, 1, padding[0], padding[1], stride, 1, flat_cs, kh, kw)
    if cin_layout is None:
        cin_layout = [(0, cin, 0)]
    cin_pad = _round_up(max(d + (e - s) for s, e, d in cin_layout), 32)
    wp = torch.zeros(cout_pad, kh * kw, cin_pad)
    wt = weight.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    for s, e, d in cin_layout:
        wp[:cout, :, d:d + (e - s)] = wt[:, :, s:e]
    return PackedConv(wp.reshape(cout_pad, kh * kw * cin_pad).contiguous().to(DEV), b.to(DEV), cout, cout_pad,
                      cin_pad, kh, kw, padding[0], padding[1], stride, 0, 0, kh, kw)


def repack_conv_(pc, new):
    """Copy the packed layer `new` (pack_conv of other values of the same layer) into the device tensors of `pc`, IN PLACE:
    parameter structs and captured launches that hold pc's addresses then read the new values.  Every form pc has built so far
    (fp32 rows, the bf16 split, fragment orders, the fp16 plane) is rewritten."""
    assert pc.wgt.shape == new.wgt.shape and pc.bias.shape == new.bias.shape
    pc.wgt.copy_(new.wgt)
    pc.bias.copy_(new.bias)
    pc.wgt_hi.copy_(new.wgt_hi)
    pc.wgt_lo.copy_(new.wgt_lo)
    for key, t in (pc._frag or {}).items():
        t.copy_(new.frag_mx() if key == "mx" else new.frag(1, f16=True) if key == "f16" else new.frag(key))
    if pc._f16 is not None:
        pc._f16.copy_(new.wgt_f16())


def fold_bn(weight, bias, bn_w, bn_b, mean, var, eps=1e-5):
    """Eval-mode BatchNorm folded into the preceding conv (extractor.py:22-26)."""
    s = (bn_w.double() / torch.sqrt(var.double() + eps))
    w = (weight.double() * s[:, None, None, None]).float()
    b = ((bias.double() - mean.double()) * s + bn_b.double()).float()
    return w, b


# PRECISION (conv_select's).  "f16mx8" (round 4): fp16 main term + two block-scaled fp8 cross terms -- an fp32-emulating product in two
# matrix-pipe passes instead of bf16x3's three (woft_conv_params.wgt_mx); layers whose kernel has no such instance run in bf16x3
#
# Developer switches of the kernel selection (conv_select.Switches): module attributes, gathered by _switches() at every call.
# which layers precision "f16mx8" actually runs in two passes: "auto" (default) = where it measured faster than bf16x3; "all" = every
# multi-tap layer of the register-streamed kernel (the kernel tests use it)
MX_LAYERS = os.environ.get("WOFT_MX_LAYERS", "auto")
SLOW_GATES = os.environ.get("WOFT_SLOW_GATES", "0") != "0"     # developer A/B: libm sigmoid / tanh in the conv epilogues
USE_HALO = os.environ.get("WOFT_HALO", "1") != "0"
USE_REGB = os.environ.get("WOFT_REGB", "1") != "0"
REGB_TY4 = os.environ.get("WOFT_REGB_TY4", "1") != "0"
USE_STEM = os.environ.get("WOFT_STEM", "1") != "0"        # 7x7 / stride-2 first layer on conv_stem.hip (0: gather kernel)
USE_1X1 = os.environ.get("WOFT_1X1", "1") != "0"          # wide 1x1 layers on conv_1x1.hip (0: gather kernel)
HALO_MIN_BLOCKS = int(os.environ.get("WOFT_HALO_MIN_BLOCKS", "400"))
WH_HALO = int(os.environ.get("WOFT_WH_HALO", "2"))
TILE_MIN_BLOCKS = int(os.environ.get("WOFT_TILE_MIN_BLOCKS", "400"))
assert conv_select.EPI_FLOWHEAD == _lib.EPI_FLOWHEAD


def _switches():
    return conv_select.Switches(USE_HALO, USE_REGB, REGB_TY4, USE_STEM, USE_1X1, WH_HALO, HALO_MIN_BLOCKS, TILE_MIN_BLOCKS,
                                MX_LAYERS, os.environ.get("WOFT_MX_ZR", "12"))


# ------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------
def select_conv(x, pc, epi=_lib.EPI_LINEAR, x2=None, stats=None, ho=None, wo=None, tiles=None, cout=None, precision=0, halo=None,
                in_norm=0, bias_map=None, wh0=None, **_):
    """conv_select.select() for the layer conv_params(x, pc, out, ...) would build, from the same arguments (the others are ignored)."""
    if ho is None or wo is None:
        ho, wo = pc.out_hw(x.h, x.w)
    layer = conv_select.Layer(x.n, x.h, x.w, ho, wo, pc.taps_y, pc.taps_x, pc.stride, pc.pad_y, pc.pad_x, pc.cin_pad,
                              cout or pc.cout, pc.cout_pad, pc.flat, x.cs, x2 is not None, stats is not None, int(in_norm or 0),
                              bias_map is not None, wh0 is not None, epi)
    return conv_select.select(layer, PRECISION.get(precision, precision), _switches(), tiles, halo)


def conv_params(x, pc, out, co_off=0, epi=_lib.EPI_LINEAR, x2=None, c_split=0, e0=None, e1=None, out1=None,
                split=0, alpha=1.0, stats=None, ho=None, wo=None, tiles=None, cout=None, precision=0, halo=None,
                in_norm=0, in_stats=None, bias_map=None, x2_off=0, wh0=None):
    """Build (and keep alive) a woft_conv_params for `out[:, co_off:co_off+cout] = epi(conv(x))` on the kernel instance that
    conv_select.select() picks (tiles, halo: its overrides).
    in_norm = 1 / 2 with in_stats = (mean, rstd): x is a RAW conv output, InstanceNorm (2: + ReLU) applied while loading where
    the kernel can (p.in_norm on the result; else the caller falls back to woft_inorm_apply).
    wh0 = (lookup Act, mean, fragments (pack_wh0_frags), bias, index | None): the weight head's first conv is evaluated inside
    this launch from the lookup windows and x is not read."""
    if ho is None or wo is None:
        ho, wo = pc.out_hw(x.h, x.w)
    sel = select_conv(x, pc, epi=epi, x2=x2, stats=stats, ho=ho, wo=wo, tiles=tiles, cout=cout, precision=precision, halo=halo,
                      in_norm=in_norm, bias_map=bias_map, wh0=wh0)
    p = ConvParams()
    p.in0, p.cs0 = ptr(x.t), x.cs
    if x2 is not None:                  # (x2_off: first channel of x2 used as the second source)
        p.in1, p.cs1, p.c_split = x2.t.data_ptr() + 4 * x2_off, x2.cs, c_split
    else:
        p.in1, p.cs1, p.c_split = None, 0, pc.cin_pad
    p.n_img, p.h, p.w, p.ho, p.wo = x.n, x.h, x.w, ho, wo
    p.taps_y, p.taps_x, p.stride, p.pad_y, p.pad_x = pc.taps_y, pc.taps_x, pc.stride, pc.pad_y, pc.pad_x
    p.cin_pad, p.flat = pc.cin_pad, pc.flat
    p.wgt, p.bias, p.alpha = ptr(pc.wgt), ptr(pc.bias), alpha
    p.wgt_hi, p.wgt_lo, p.precision = ptr(pc.wgt_hi), ptr(pc.wgt_lo), sel.precision
    if PRECISION.get(precision, precision) == conv_select.FP16:    # fp16 operands: the weight plane holds fp16 values
        p.wgt_hi, p.wgt_lo = ptr(pc.wgt_f16()), None
    p.wgt_frag = p.wgt_mx = None
    if KERNELS[sel.kernel].weights == conv_select.FRAG:  # weights in MFMA-fragment order (conv_regb.hip, conv_1x1.hip)
        p.wgt_frag = ptr(pc.frag(2 if sel.precision == conv_select.BF16X3 else 1,
                                 f16=sel.precision in (conv_select.FP16, conv_select.F16MX8)))
        if sel.precision == conv_select.F16MX8:
            p.wgt_mx = ptr(pc.frag_mx())
    p.cout, p.cout_pad = (cout or pc.cout), sel.cout_pad
    p.out, p.ldo, p.co_off = ptr(out.t), out.cs, co_off
    p.out_w, p.out_pitch = (-12346 if SLOW_GATES else 0), 0
    p.epi, p.split = epi, split
    p.e0, p.lde0 = (ptr(e0.t), e0.cs) if e0 is not None else (None, 0)
    p.e1, p.lde1 = (ptr(e1.t), e1.cs) if e1 is not None else (None, 0)
    p.out1, p.ldo1 = (ptr(out1.t), out1.cs) if out1 is not None else (None, 0)
    p.tile_m, p.tile_n, p.halo = sel.tile_m, sel.tile_n, sel.kernel
    p.bias_map, p.ld_bias_map = (ptr(bias_map.t), bias_map.cs) if bias_map is not None else (None, 0)
    p.in_norm, p.in_mean, p.in_rstd = (sel.in_norm, ptr(in_stats[0]), ptr(in_stats[1])) if sel.in_norm else (0, None, None)
    if stats is not None:
        assert stats[0].numel() >= 2 * sel.m_tiles * pc.cout_pad
        p.stat_sum, p.stat_sq = ptr(stats[0]), ptr(stats[1])
    else:
        p.stat_sum, p.stat_sq = None, None
    if wh0 is not None:
        lk, mean, frag, b0, index = wh0
        p.wh0_lookup, p.wh0_ld, p.wh0_mean = ptr(lk.t), lk.cs, ptr(mean)
        p.wh0_w, p.wh0_bias, p.wh0_index = ptr(frag), ptr(b0), (ptr(index) if index is not None else None)
    p._keep = (x, x2, pc, out, e0, e1, out1, stats, in_stats, bias_map, wh0, p.wgt_frag and pc._frag)
    p._m, p._m_tiles = x.n * ho * wo, sel.m_tiles
    return p


def pack_wh0_frags(w0, planes):
    """First conv of the weight head (128, 5, 3, 3) (weighted_raft.py:336) -> bf16 MFMA A fragments
    [4 chunks][3 K steps][planes][64 lanes][8] (woft_conv_params.wh0_w): k = (3 ky + kx) * 5 + ci, 45 -> 48."""
    k = torch.zeros(128, 48)
    k[:, :45] = w0.detach().float().cpu().permute(0, 2, 3, 1).reshape(128, 45)
    k = k.reshape(4, 32, 3, 2, 8).permute(0, 2, 3, 1, 4).reshape(4, 3, 64, 8)      # lane = 32 * (k half) + row
    hi = k.to(torch.bfloat16)
    pl = [hi] + ([(k - hi.float()).to(torch.bfloat16)] if planes == 2 else [])
    return torch.stack(pl, dim=2).contiguous().to(DEV)


def pack_flowhead_frags(w2, planes, f16=False):
    """FlowHead.conv2 weight (2, C, 3, 3) (update.py:11) -> bf16 MFMA B fragments [C/32 bands][2 k halves][planes][64 lanes][8]
    for WOFT_EPI_FLOWHEAD: lane = 32 * hh + j, column j = (3 ky + kx) * 2 + o (18 of 32 used), element e = channel
    32 band + 16 (k half) + 8 hh + e."""
    w2 = w2.detach().float().cpu()
    c = w2.shape[1]
    assert w2.shape[0] == 2 and tuple(w2.shape[2:]) == (3, 3) and c % 32 == 0
    cols = torch.zeros(32, c)
    cols[:18] = w2.permute(2, 3, 0, 1).reshape(18, c)                 # row j = (ky * 3 + kx) * 2 + o
    f = cols.reshape(32, c // 32, 2, 2, 8).permute(1, 2, 3, 0, 4).reshape(c // 32, 2, 64, 8)   # band, k half, (hh, j), e
    if f16:                             # precision "fp16": one plane of fp16 values in the 16-bit containers
        return f.to(torch.float16).view(torch.bfloat16).reshape(c // 32, 2, 1, 64, 8).contiguous().to(DEV)
    hi = f.to(torch.bfloat16)
    pl = [hi] + ([(f - hi.float()).to(torch.bfloat16)] if planes == 2 else [])
    return torch.stack(pl, dim=2).contiguous().to(DEV)


def flowhead_params(x, pc, part, frags, **kw):
    """conv_params for FlowHead.conv1 with the second conv folded into its epilogue (WOFT_EPI_FLOWHEAD), or None when the
    layer does not run on the register-streamed kernel (8 x 16 pixel tiles) here.  part: (planes * n_pix, >= 20) fp32."""
    p = conv_params(x, pc, Act(part, 1, x.h, x.w, 18), epi=_lib.EPI_FLOWHEAD, **kw)
    if Kernel(p.halo) is not Kernel.REGB_8X16 or pc.cout % 32 != 0:
        return None
    n_planes = p.cout_pad // p.tile_n
    assert part.shape[0] >= n_planes * x.n_pix and part.shape[1] >= 20 and x.n == 1
    p.e0, p.lde0 = ptr(frags), 0
    p._keep = p._keep + (part, frags)
    p._n_planes = n_planes
    return p


def flow_head_gather(part, n_planes, h, w, bias2, delta, coords, flow4=None, flow_cat=None, ld_cat=0):
    check(_lib.load().woft_flow_head_gather(ptr(part), n_planes, part.shape[1], h, w, ptr(bias2), ptr(delta.t), delta.cs,
                                            ptr(coords), ptr(flow4), ptr(flow_cat), ld_cat, stream_ptr()),
          "woft_flow_head_gather")


def run_conv_pair(a, b):
    check(_lib.load().woft_conv2d_pair(C.byref(a), C.byref(b), stream_ptr()), "woft_conv2d_pair")


def run_conv(p):
    check(_lib.load().woft_conv2d(C.byref(p), stream_ptr()), "woft_conv2d")


def conv2d(x, pc, c_out_stride=None, **kw):
    """Convenience: allocate the output and run.  Returns Act."""
    ho, wo = pc.out_hw(x.h, x.w)
    out = kw.pop("out", None) or new_act(x.n, ho, wo, pc.cout, cs=c_out_stride or _round_up(pc.cout, 4), zero=True)
    p = conv_params(x, pc, out, ho=ho, wo=wo, **kw)
    run_conv(p)
    return out


def inorm_ws(device="cuda"):
    """Scratch of woft_inorm_finalize (cross-workgroup partial sums + ticket), zeroed once; one per stream of calls."""
    return torch.zeros(int(_lib.load().woft_inorm_ws_bytes()), dtype=torch.uint8, device=device)


def inorm_finalize(stats, n_part, ld, channels, count, mean, rstd, eps=1e-5, channels_pad=None, ws=None):
    check(_lib.load().woft_inorm_finalize(ptr(stats[0]), ptr(stats[1]), n_part, ld, channels, channels_pad or channels,
                                          count, eps, ptr(mean), ptr(rstd), ptr(ws), stream_ptr()), "woft_inorm_finalize")


def inorm_apply(x, mean, rstd, out, mode, res=None, res_stats=None, res_mode=0):
    """res_mode 1 / 2: `res` is a raw conv output, normalised (2: + ReLU) with res_stats = (mean, rstd) inside the kernel."""
    assert out.cs == x.cs and (res is None or res.cs == x.cs)
    rm, rr = res_stats if res_stats is not None else (None, None)
    check(_lib.load().woft_inorm_apply(ptr(x.t), ptr(mean), ptr(rstd), ptr(res.t) if res is not None else None,
                                       ptr(rm), ptr(rr), res_mode, ptr(out.t), x.n_pix, x.cs, mode, stream_ptr()),
          "woft_inorm_apply")


class PyramidArgs:
    """Pointer tables of woft_feature_pyramid, built once (kept alive with the tensors they point to)."""
    def __init__(self, maps, splits, terms):
        import ctypes
        self.maps, self.splits, self.terms = maps, splits, terms
        self.levels = len(maps)
        assert 1 <= self.levels <= 4 and len(splits) == self.levels and all(m.cs == maps[0].cs == m.c for m in maps)
        for l in range(1, self.levels):
            assert (maps[l].h, maps[l].w) == (maps[l - 1].h // 2, maps[l - 1].w // 2)
        self.pooled = (ctypes.c_void_p * 3)(*[maps[l].t.data_ptr() if l < self.levels else None for l in range(1, 4)])
        self.split = (ctypes.c_void_p * 4)(*[splits[l].data_ptr() if l < self.levels else None for l in range(4)])


def feature_pyramid(a):
    """maps[0] -> pooled maps[1:] (avgpool2 chained) and every level's split correlation operand, one launch."""
    m = a.maps[0]
    check(_lib.load().woft_feature_pyramid(ptr(m.t), m.h, m.w, m.cs, a.levels, a.pooled, a.split, a.terms, stream_ptr()),
          "woft_feature_pyramid")


def preprocess(img_u8, out, hp, wp, pad_top, pad_left):
    h, w = img_u8.shape[:2]
    check(_lib.load().woft_preprocess_bgr_u8(ptr(img_u8), h, w, ptr(out.t), hp, wp, pad_top, pad_left, stream_ptr()),
          "woft_preprocess_bgr_u8")


def avgpool2(x, out):
    check(_lib.load().woft_avgpool2_nhwc(ptr(x.t), x.h, x.w, x.cs, ptr(out.t), stream_ptr()), "woft_avgpool2_nhwc")


def split_bf16(x, hi, lo=None):
    check(_lib.load().woft_split_bf16(ptr(x), x.numel(), ptr(hi), ptr(lo), stream_ptr()), "woft_split_bf16")


def conv3x3_narrow(x, pc, out, co_off=0):
    """3x3 / stride 1 / pad 1 conv with cout <= 2 in exact fp32 (woft_conv3x3_narrow); x, out: Act."""
    assert (pc.taps_y, pc.taps_x, pc.stride, pc.pad_y, pc.pad_x, pc.flat) == (3, 3, 1, 1, 1, 0) and pc.cout <= 2
    assert out.n == x.n and out.h == x.h and out.w == x.w
    check(_lib.load().woft_conv3x3_narrow(ptr(x.t), x.cs, x.n, x.h, x.w, pc.cin_pad, ptr(pc.wgt), ptr(pc.bias), pc.cout,
                                          ptr(out.t), out.cs, co_off, stream_ptr()), "woft_conv3x3_narrow")


def flow_head_update(x, pc, delta, coords, flow4=None, flow_cat=None, ld_cat=0):
    """conv3x3_narrow (2 channels -> delta) + coords_update in one launch (woft_flow_head_update)."""
    assert narrow_ok(x, pc) and pc.cout == 2 and x.n == 1 and coords.shape[0] == x.h * x.w
    check(_lib.load().woft_flow_head_update(ptr(x.t), x.cs, x.h, x.w, pc.cin_pad, ptr(pc.wgt), ptr(pc.bias), ptr(delta.t),
                                            delta.cs, ptr(coords), ptr(flow4), ptr(flow_cat), ld_cat, stream_ptr()),
          "woft_flow_head_update")


def narrow_ok(x, pc):
    """True when woft_conv3x3_narrow applies to this layer."""
    return ((pc.taps_y, pc.taps_x, pc.stride, pc.pad_y, pc.pad_x, pc.flat) == (3, 3, 1, 1, 1, 0) and pc.cout <= 2
            and pc.cin_pad in (128, 256) and x.cs >= pc.cin_pad)


def make_lookup_otf_params(f1s, f2s, dims, hf, wf, k, coords, out, radius, terms):
    """Volume-free lookup (woft_corr_lookup_otf): f1s / f2s[l] split feature rows (row-major), dims[l] = (h, w)."""
    p = LookupOtfParams()
    p.f1 = ptr(f1s)
    for l, (t, (h, w)) in enumerate(zip(f2s, dims)):
        p.f2[l], p.h[l], p.w[l] = ptr(t), h, w
    p.levels, p.radius, p.terms = len(f2s), radius, terms
    p.hf, p.wf, p.k = hf, wf, k
    p.alpha = 1.0 / math.sqrt(float(k))
    p.coords, p.out, p.ldo = ptr(coords), ptr(out), out.shape[1]
    p._keep = (f1s, f2s, coords, out)
    return p


def run_lookup_otf(p):
    check(_lib.load().woft_corr_lookup_otf(C.byref(p), stream_ptr()), "woft_corr_lookup_otf")


# ---- correlation band (include/woft_hip.h: woft_lookup_band_params; mirrored here, checked against woft_corr_band_geometry) ----
BAND_M0, BAND_LD = 3, 16
BAND_INSTANCES = ((4, 256), (3, 128))        # (radius, k) pairs the band kernels are built for: the volume-free lookup's


def band_m(l):
    """m_l = ceil(m_0 / 2^l): how far floor(coords / 2^l) may lie from floor(p / 2^l), in cells, for a hit."""
    return (BAND_M0 + (1 << l) - 1) >> l


def band_geometry(radius, levels):
    """-> (m, w, row_off, rows): per level the margin m_l, the band's width W_l = 2 (radius + 1 + m_l) and its first row; rows per
    source pixel.  band[(pixel * rows + row_off[l] + bx) * BAND_LD + by] is the correlation of the pixel p = (x, y) with cell
    (floor(x / 2^l) - radius - m_l + bx, floor(y / 2^l) - radius - m_l + by) of level l."""
    m = [band_m(l) for l in range(levels)]
    w = [2 * (radius + 1 + ml) for ml in m]
    off = [sum(w[:l]) for l in range(levels)]
    return m, w, off, sum(w)


def band_hit(cx, cy, x, y, levels):
    """The band lookup's per-pixel predicate (the kernel ANDs it over the valid pixels of an 8 x 8 block): floor(coords / 2^l)
    within +-m_l of floor(p / 2^l) on both axes, at every level."""
    for l in range(levels):
        s = 1.0 / (1 << l)
        if abs(math.floor(cx * s) - (x >> l)) > band_m(l) or abs(math.floor(cy * s) - (y >> l)) > band_m(l):
            return False
    return True


def make_lookup_band_params(otf, band, miss, miss_count):
    """woft_lookup_band_params around a copy of a volume-free lookup's struct (its need / fh_* / roi_* / smp_* included)."""
    p = LookupBandParams()
    C.memmove(C.byref(p), C.byref(otf), C.sizeof(LookupOtfParams))     # (the embedded struct comes first)
    p.band, p.miss, p.miss_count = ptr(band), ptr(miss), ptr(miss_count)
    p._keep = (getattr(otf, "_keep", None), band, miss, miss_count)
    return p


def run_band_build(p):
    check(_lib.load().woft_corr_band_build(C.byref(p), stream_ptr()), "woft_corr_band_build")


def run_lookup_band(p):
    check(_lib.load().woft_corr_lookup_band(C.byref(p), stream_ptr()), "woft_corr_lookup_band")


def run_conv1x1_band(c1, f1, bp):
    """convc1 with the band lookup's sampling inside its launch, convf1 (or None) on the workgroups behind (woft_conv1x1_band);
    bp: the band lookup's struct of the iteration, launched before with defer_samples = 1 and followed by its fallback."""
    check(_lib.load().woft_conv1x1_band(C.byref(c1), C.byref(f1) if f1 is not None else None, C.byref(bp), stream_ptr()),
          "woft_conv1x1_band")


def split_bf16_lines(x, out):
    """x fp32 [rows][k] -> out bf16 [rows][2k]: per 32 values one 128-byte line [hi | lo] (woft_split_bf16_lines)."""
    check(_lib.load().woft_split_bf16_lines(ptr(x), x.numel(), ptr(out), stream_ptr()), "woft_split_bf16_lines")


def features_record_floats(n_pix, fdim, hdim, cdim):
    """Floats of a frame-features record: [n_pix x fdim | n_pix x hdim | n_pix x cdim] (woft_features_pack)."""
    return n_pix * (fdim + hdim + cdim)


def features_pack(f1rows, net, xbuf, n_pix, dims, record):
    """The first n_pix rows of f1rows (fnet map), of net and of the first dims[2] channels of xbuf -> record, one launch
    (woft_features_pack).  dims = (fdim, hdim, cdim); the tensors are 2-D fp32 with contiguous rows."""
    fdim, hdim, cdim = dims
    assert record.dtype == torch.float32 and record.is_contiguous() and record.numel() == features_record_floats(n_pix, *dims)
    assert f1rows.shape[0] >= n_pix and net.shape[0] >= n_pix and xbuf.shape[0] >= n_pix
    check(_lib.load().woft_features_pack(ptr(f1rows), f1rows.stride(0), ptr(net), net.stride(0), ptr(xbuf), xbuf.stride(0),
                                         n_pix, fdim, hdim, cdim, ptr(record), stream_ptr()), "woft_features_pack")


def features_unpack(record, n_pix, dims, fmap, fmap_split=None, net=None, xbuf=None, inp_c=None):
    """record -> the first n_pix rows of fmap; with net, xbuf and inp_c (the source role) also those and, with fmap_split, the
    fnet map's [hi | lo] lines -- one launch (woft_features_unpack).  Without them (the target role) fmap alone."""
    fdim, hdim, cdim = dims
    assert record.dtype == torch.float32 and record.is_contiguous() and record.numel() == features_record_floats(n_pix, *dims)
    assert fmap.shape[0] >= n_pix and all(t is None or t.shape[0] >= n_pix for t in (fmap_split, net, xbuf, inp_c))
    ld = lambda t: 0 if t is None else t.stride(0)
    check(_lib.load().woft_features_unpack(ptr(record), n_pix, fdim, hdim, cdim, ptr(fmap), ld(fmap), ptr(fmap_split), ptr(net),
                                           ld(net), ptr(xbuf), ld(xbuf), ptr(inp_c), ld(inp_c), stream_ptr()),
          "woft_features_unpack")


def corr_gemm_bf16(a, b, m, n, alpha, out, terms):
    """out[:m, :n] = alpha * A B^T on pre-split bf16 operands (rows padded to 128); see woft_corr_gemm_bf16.
    out: float32, or bfloat16 for the bf16-storage volume."""
    k = a.shape[1] // 2 if terms == 3 else a.shape[1]
    assert out.dtype in (torch.float32, torch.bfloat16)
    check(_lib.load().woft_corr_gemm_bf16(ptr(a), ptr(b), m, n, a.shape[0], b.shape[0], k, float(alpha), ptr(out),
                                          out.shape[1], terms, int(out.dtype == torch.bfloat16), stream_ptr()),
          "woft_corr_gemm_bf16")


def corr_volume(f1, f2_rows, n_q, out, alpha, precision=0, f2_hi=None, f2_lo=None):
    """out[p][q] = alpha * <f1[p], f2_rows[q]>, q < n_q (rows of f2 already in the order the volume wants).
    f1: Act (P, C); f2_rows: tensor (rows_pad, C) zero padded to a multiple of 128 rows;
    f2_hi / f2_lo: its bf16 split (ops.split_bf16) for the bf16 precisions."""
    p = ConvParams()
    p.in0, p.cs0, p.in1, p.cs1, p.c_split = ptr(f1.t), f1.cs, None, 0, f1.cs
    p.n_img, p.h, p.w, p.ho, p.wo = 1, f1.h, f1.w, f1.h, f1.w
    p.taps_y = p.taps_x = p.stride = 1
    p.pad_y = p.pad_x = 0
    p.cin_pad, p.flat = f1.cs, 0
    p.wgt, p.bias, p.alpha = ptr(f2_rows), None, alpha
    p.wgt_hi, p.wgt_lo, p.precision = ptr(f2_hi), ptr(f2_lo), PRECISION.get(precision, precision)
    p.cout, p.cout_pad = n_q, f2_rows.shape[0]
    p.out, p.ldo, p.co_off = ptr(out), out.shape[1], 0
    p.out_w, p.out_pitch = 0, 0
    p.epi = _lib.EPI_LINEAR
    p.tile_m, p.tile_n = (128, 128) if f2_rows.shape[0] % 128 == 0 else (128, 64)
    p.halo = Kernel.GATHER
    p._keep = (f1, f2_rows, out, f2_hi, f2_lo)
    return p


def tiled_dims(h, w, tw=4):
    """(tile rows, tile cols, elements per plane) of an h x w map in the volume layout of 4 x 4 tiles."""
    ht, wt = (h + 3) // 4, (w + tw - 1) // tw
    return ht, wt, ht * wt * 4 * tw


def tile_rows(x, out):
    """x: Act (1, h, w, c) -> out rows in 4x4-tile order (first ht*wt*16 rows of `out`)."""
    check(_lib.load().woft_tile_rows(ptr(x.t), x.h, x.w, x.cs, ptr(out), stream_ptr()), "woft_tile_rows")


def tile_planes(planes, tw=4):
    """(P, h, w) tensor of per-source-pixel planes -> (P, ht*wt*4*tw) in the tiled layout (test helper)."""
    P, h, w = planes.shape
    ht, wt, n = tiled_dims(h, w, tw)
    pad = torch.zeros(P, ht * 4, wt * tw, dtype=planes.dtype, device=planes.device)
    pad[:, :h, :w] = planes
    return pad.reshape(P, ht, 4, wt, tw).permute(0, 1, 3, 2, 4).reshape(P, n).contiguous()


def untile_planes(vol, h, w, tw=4):
    """inverse of tile_planes: (P, >= ht*wt*4*tw) -> (P, h, w)."""
    ht, wt, n = tiled_dims(h, w, tw)
    P = vol.shape[0]
    return vol[:, :n].reshape(P, ht, wt, 4, tw).permute(0, 1, 3, 2, 4).reshape(P, ht * 4, wt * tw)[:, :h, :w]


def make_lookup_params(vols, dims, coords, out, radius):
    """vols[l]: (P, plane_l) tiled volumes (4 x 4 tiles), all float32 or all bfloat16; dims[l] = (H_l, W_l)."""
    p = LookupParams()
    assert len({v.dtype for v in vols}) == 1 and vols[0].dtype in (torch.float32, torch.bfloat16)
    p.vol_bf16 = int(vols[0].dtype == torch.bfloat16)
    for l, v in enumerate(vols):
        p.vol[l] = ptr(v)
        p.ht[l], p.wt[l], n = tiled_dims(*dims[l])
        assert v.shape[1] >= n
        p.plane[l] = v.shape[1]
    p.levels, p.radius = len(vols), radius
    p.coords, p.n_pix, p.out, p.ldo = ptr(coords), coords.shape[0], ptr(out), out.shape[1]
    p._keep = (vols, coords, out)
    return p


def run_lookup(p):
    check(_lib.load().woft_corr_lookup(C.byref(p), stream_ptr()), "woft_corr_lookup")


def coords_init(coords, hf, wf, flow4=None, flow_cat=None, ld_cat=0):
    check(_lib.load().woft_coords_init(ptr(coords), hf, wf, ptr(flow4), ptr(flow_cat), ld_cat, stream_ptr()),
          "woft_coords_init")


def coords_init_flow(coords, flow_init, hf, wf, flow4=None, flow_cat=None, ld_cat=0):
    """coords = grid + flow_init, flow4 / flow_cat = flow_init itself (woft_coords_init_flow).  flow_init: contiguous (2, hf, wf)
    fp32 device tensor, 1/8-resolution pixels of the padded image."""
    assert flow_init.dtype == torch.float32 and flow_init.is_contiguous() and tuple(flow_init.shape) == (2, hf, wf)
    check(_lib.load().woft_coords_init_flow(ptr(coords), ptr(flow_init), hf, wf, ptr(flow4), ptr(flow_cat), ld_cat,
                                            stream_ptr()), "woft_coords_init_flow")


def forward_interpolate(flow, out=None):
    """forward_interpolate (raft_core/utils/utils.py:28-56) of a contiguous (2, hf, wf) fp32 device tensor -> `out` (a new
    tensor by default; never `flow` itself): woft_forward_interpolate -- exact nearest valid landing point per cell, lowest
    point index on a tie, zeros without any valid point."""
    assert flow.dtype == torch.float32 and flow.is_contiguous() and flow.dim() == 3 and flow.shape[0] == 2
    if out is None:
        out = torch.empty_like(flow)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == flow.shape
    check(_lib.load().woft_forward_interpolate(ptr(flow), flow.shape[1], flow.shape[2], ptr(out), stream_ptr()),
          "woft_forward_interpolate")
    return out


def _f32c(t, *shape):
    return t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda and (not shape or tuple(t.shape) == shape)


def sample_bilinear(data, x, y, out=None):
    """bilinear_interpolate_torch (utils/interpolation.py:92-133) of a contiguous (C, H, W) fp32 device tensor at the N points
    (x, y) -> (C, N): woft_sample_bilinear -- the reference's fp32 result bit for bit, its zeros on and beyond the last row /
    column included."""
    assert data.dim() == 3 and _f32c(data) and x.dim() == 1 and _f32c(x) and _f32c(y, *x.shape)
    c, h, w = data.shape
    n = x.shape[0]
    if out is None:
        out = torch.empty((c, n), dtype=torch.float32, device=data.device)
    assert _f32c(out, c, n)
    check(_lib.load().woft_sample_bilinear(ptr(data), c, h, w, ptr(x), ptr(y), n, ptr(out), stream_ptr()), "woft_sample_bilinear")
    return out


def flow_chain(flow_ab, flow_bc, out=None):
    """flow_ab + flow_bc sampled at pixel + flow_ab (edge-exact bilinear; NaN where that point leaves the frame) of two contiguous
    (2, H, W) fp32 device tensors -> `out` (a new tensor by default; not flow_bc): woft_flow_chain."""
    assert flow_ab.dim() == 3 and flow_ab.shape[0] == 2 and _f32c(flow_ab) and _f32c(flow_bc, *flow_ab.shape)
    if out is None:
        out = torch.empty_like(flow_ab)
    assert _f32c(out, *flow_ab.shape) and out.data_ptr() != flow_bc.data_ptr()
    check(_lib.load().woft_flow_chain(ptr(flow_ab), ptr(flow_bc), flow_ab.shape[1], flow_ab.shape[2], ptr(out), stream_ptr()),
          "woft_flow_chain")
    return out


def flow_fb(flow_ab, flow_ba, alpha=0.01, beta=0.5, err=None, ok=None, want_err=True, want_ok=True):
    """Forward-backward check of two contiguous (2, H, W) fp32 device tensors -> (err (H, W) | None, ok (H, W) 0/1 floats | None):
    woft_flow_fb.  err = |flow_ab + flow_ba(pixel + flow_ab)|, ok = err^2 <= alpha * (|flow_ab|^2 + |flow_ba(..)|^2) + beta;
    a pixel whose flow leaves the frame: err = +inf, ok = 0."""
    assert flow_ab.dim() == 3 and flow_ab.shape[0] == 2 and _f32c(flow_ab) and _f32c(flow_ba, *flow_ab.shape)
    h, w = flow_ab.shape[1:]
    if err is None and want_err:
        err = torch.empty((h, w), dtype=torch.float32, device=flow_ab.device)
    if ok is None and want_ok:
        ok = torch.empty((h, w), dtype=torch.float32, device=flow_ab.device)
    assert (err is None or (_f32c(err) and err.numel() == h * w)) and (ok is None or (_f32c(ok) and ok.numel() == h * w))
    check(_lib.load().woft_flow_fb(ptr(flow_ab), ptr(flow_ba), h, w, float(alpha), float(beta), ptr(err), ptr(ok), stream_ptr()),
          "woft_flow_fb")
    return err, ok


def _post_h9(post_H):
    """A closing homography -> the 9 doubles woft_flow_chain_fold_window takes (h8 = 1: normalised here); None -> NULL."""
    if post_H is None:
        return None
    Hm = np.asarray(post_H, dtype=np.float64)
    if Hm.shape != (3, 3) or not np.all(np.isfinite(Hm)) or Hm[2, 2] == 0.0:
        raise ValueError(f"flow_chain_fold_window: post_H must be a finite 3 x 3 matrix with a non-zero last entry, got {post_H!r}")
    Hm = Hm / Hm[2, 2]
    Hm[2, 2] = 1.0
    if not np.all(np.isfinite(Hm)):
        raise ValueError(f"flow_chain_fold_window: post_H does not normalise to a finite matrix, got {post_H!r}")
    return (C.c_double * 9)(*Hm.ravel().tolist())


def _flow_chain_fold(name, best, prev, step_flow, step_wlogit, step_mlogit, k, rects, post_H, vis_thr, unit_cost, first):
    """The one body of flow_chain_fold and flow_chain_fold_window (`name`: the caller's, for messages).  rects: (template_rect,
    step_rect), or None: whole frames -- every plane has the step flow's size, and the entry point is woft_flow_chain_fold."""
    assert step_flow.dim() == 3 and step_flow.shape[0] == 2 and _f32c(step_flow)
    if rects is None:
        th, tw = sh, sw = step_flow.shape[1:]
    else:
        (ty0, tx0, th, tw), (sy0, sx0, sh, sw) = ([int(v) for v in r] for r in rects)
        assert tuple(step_flow.shape[1:]) == (sh, sw), f"step flow {tuple(step_flow.shape)} is not on the step rect {(sh, sw)}"
    n, ns = th * tw, sh * sw
    plane = lambda t, m: t is not None and _f32c(t) and t.numel() == m
    assert (step_wlogit is None or plane(step_wlogit, ns)) and (step_mlogit is None or plane(step_mlogit, ns))
    if prev is not None:
        assert len(prev) == 3 and _f32c(prev[0], 2, th, tw) and plane(prev[1], n) and plane(prev[2], n)
    k, vis_thr, unit_cost = int(k), float(vis_thr), float(unit_cost)
    if not 0 <= k <= 127:
        raise ValueError(f"{name}: k must be in [0, 127], got {k}")
    if not (0.0 <= vis_thr <= 1.0) or not (unit_cost >= 0.0):
        raise ValueError(f"{name}: vis_thr must be in [0, 1] and unit_cost >= 0, got {vis_thr!r}, {unit_cost!r}")
    h9 = None if rects is None else _post_h9(post_H)
    if best is None:
        assert first, f"{name}: without a running best the fold must be the first"
        new = lambda dtype, *s: torch.empty(s, dtype=dtype, device=step_flow.device)
        best = (new(torch.float32, 2, th, tw), new(torch.float32, th, tw), new(torch.float32, th, tw), new(torch.int32, th, tw))
    bf, bc, bv, bs = best
    assert _f32c(bf, 2, th, tw) and plane(bc, n) and plane(bv, n)
    assert bs.dtype == torch.int32 and bs.is_contiguous() and bs.is_cuda and bs.numel() == n
    pf, pc, pv = prev if prev is not None else (None, None, None)
    if rects is None:
        rc = _lib.load().woft_flow_chain_fold(ptr(pf), ptr(pc), ptr(pv), ptr(step_flow), ptr(step_wlogit), ptr(step_mlogit), th, tw,
                                              unit_cost, vis_thr, k, int(bool(first)), ptr(bf), ptr(bc), ptr(bv), ptr(bs), stream_ptr())
    else:
        rc = _lib.load().woft_flow_chain_fold_window(ptr(pf), ptr(pc), ptr(pv), th, tw, ty0, tx0, ptr(step_flow), ptr(step_wlogit),
                                                     ptr(step_mlogit), sh, sw, sy0, sx0, h9, unit_cost, vis_thr, k, int(bool(first)),
                                                     ptr(bf), ptr(bc), ptr(bv), ptr(bs), stream_ptr())
    check(rc, "woft_" + name)
    return best


def flow_chain_fold(best, prev, step_flow, step_wlogit=None, step_mlogit=None, k=0, vis_thr=0.5, unit_cost=1.0, first=False):
    """One candidate chain folded into the running per-pixel best (woft_flow_chain_fold).
    best = (flow (2, H, W), cost, vis (H*W fp32 each), sel (H*W int32)): contiguous device tensors, updated in place and returned;
    None allocates them (then `first` must be set).  prev = (flow, cost, vis) of the stored result template -> s, or None for
    the template itself.  step_flow (2, H, W) = the flow s -> t, step_wlogit / step_mlogit (H*W elements each, optional) its
    reliability and visibility logits.  The candidate's key is (vis < vis_thr, cost); it replaces the best where its key is
    strictly smaller, sel then holds k.  first: the best is empty and is not read."""
    return _flow_chain_fold("flow_chain_fold", best, prev, step_flow, step_wlogit, step_mlogit, k, None, None, vis_thr, unit_cost,
                            first)


def flow_chain_fold_window(best, prev, step_flow, step_wlogit=None, step_mlogit=None, k=0, template_rect=None, step_rect=None,
                           post_H=None, vis_thr=0.5, unit_cost=1.0, first=False):
    """flow_chain_fold on two rectangles (woft_flow_chain_fold_window).  template_rect = (y0, x0, rows, cols):
    the template rectangle of the best / prev planes ((2, rows, cols) flows, rows * cols elements per plane); step_rect likewise
    for step_flow (2, rows, cols) and the step's logits, the same rectangle of frames s and t.  Flows are displacements in frame
    coordinates.  post_H (3 x 3, optional): the candidate's landing is mapped through it in fp64 (normalised to h8 = 1 here).
    best = None allocates the running best (then `first` must be set); it is updated in place and returned."""
    return _flow_chain_fold("flow_chain_fold_window", best, prev, step_flow, step_wlogit, step_mlogit, k, (template_rect, step_rect),
                            post_H, vis_thr, unit_cost, first)


CHAIN_HIST = 130        # WOFT_CHAIN_HIST: one counter per candidate index 0..127, [128] invalid, [129] valid but occluded


MULTI_MAX_TARGETS = 32  # WOFT_MULTI_MAX_TARGETS: the targets of one bit plane (uint32 per pixel)


def _check_tbits(tbits, mh, mw, n_targets):
    if not 1 <= int(n_targets) <= MULTI_MAX_TARGETS:
        raise ValueError(f"n_targets must be in [1, {MULTI_MAX_TARGETS}], got {n_targets!r}")
    # (torch has no unsigned 32-bit arithmetic worth the name: the plane travels as int32 with the same bits)
    assert tbits.dtype == torch.int32 and tbits.is_contiguous() and tbits.is_cuda and tbits.numel() == mh * mw


def _chain_tc(name, flow, cost, vis, sel, mask, n_targets, vis_thr, window, want_w, mask_hw, out):
    """The one body of chain_tc, chain_tc_window, chain_tc_multi and chain_tc_multi_window (`name`: the caller's, for messages
    and for its entry point woft_<name>).  mask: with n_targets None the uint8 template mask or None, else the int32 bit plane of
    n_targets masks.  window: None, or the rectangle forms' (origin, frame_hw)."""
    assert flow.dim() == 3 and flow.shape[0] == 2 and _f32c(flow)
    h, w = flow.shape[1:]
    n = h * w
    assert all(_f32c(t) and t.numel() == n for t in (cost, vis))
    assert sel.dtype == torch.int32 and sel.is_contiguous() and sel.is_cuda and sel.numel() == n
    vis_thr = float(vis_thr)
    if not (0.0 <= vis_thr <= 1.0):
        raise ValueError(f"{name}: vis_thr must be in [0, 1], got {vis_thr!r}")
    mh, mw = mask_hw or (h, w)
    multi = n_targets is not None
    if multi:
        _check_tbits(mask, mh, mw, n_targets)
    elif mask is not None:
        assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.is_cuda and mask.numel() == mh * mw
    hist_shape = (n_targets, CHAIN_HIST) if multi else (CHAIN_HIST,)
    if out is None:
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=flow.device)
        out = (new(2, n), new(1, n) if want_w else None, new(1, n), torch.empty(hist_shape, dtype=torch.int32, device=flow.device))
    dst, wout, ok, hist = out
    if not want_w:
        wout = None
    assert _f32c(dst, 2, n) and _f32c(ok, 1, n) and (wout is None or _f32c(wout, 1, n))
    # (a single mask may go without a histogram; a multi-target one may be a view into a larger result block)
    assert hist is not None or not multi, f"{name}: a histogram is required"
    assert hist is None or (hist.dtype == torch.int32 and hist.is_contiguous() and hist.is_cuda
                            and hist.numel() == (n_targets if multi else 1) * CHAIN_HIST)
    lib, planes = _lib.load(), (ptr(flow), ptr(cost), ptr(vis), ptr(sel), ptr(mask), h, w, mh, mw)
    outs = (vis_thr, ptr(dst), ptr(wout), ptr(ok), ptr(hist), stream_ptr())
    if window is not None:
        rect = (int(window[0][0]), int(window[0][1]), int(window[1][0]), int(window[1][1]))
    if multi and window is not None:
        rc = lib.woft_chain_tc_multi_window(*planes, int(n_targets), *rect, *outs)
    elif multi:
        rc = lib.woft_chain_tc_multi(*planes, int(n_targets), *outs)
    elif window is not None:
        rc = lib.woft_chain_tc_window(*planes, *rect, *outs)
    else:
        rc = lib.woft_chain_tc(*planes, *outs)
    check(rc, "woft_" + name)
    return dst, wout, ok, hist


def chain_tc(flow, cost, vis, sel, tmask_u8, vis_thr, want_w=True, mask_hw=None, out=None):
    """A fold result as correspondences for the planar fit (woft_chain_tc) -> (dst (2, n), w (1, n) | None,
    ok (1, n), hist (130,) int32), n = H * W.  flow (2, H, W), cost, vis (n fp32 each), sel (n int32): contiguous device tensors,
    what flow_chain_fold leaves.  tmask_u8: the template mask (uint8, mask_hw = (mh, mw) >= (H, W), default the grid's size), or
    None: every pixel counts in hist.  dst = pixel + flow (NaN where the pixel has no valid chain), w = exp(-cost) (0 there;
    want_w=False: not computed), ok = 1 where valid and not (vis < vis_thr), hist[s] = masked pixels with ok = 1 and sel = s,
    hist[128] = masked invalid pixels, hist[129] = masked occluded ones.  out: the tuple of an earlier call at this size, reused."""
    return _chain_tc("chain_tc", flow, cost, vis, sel, tmask_u8, None, vis_thr, None, want_w, mask_hw, out)


def chain_tc_window(flow, cost, vis, sel, tmask_u8, vis_thr, origin, frame_hw, want_w=True, mask_hw=None, out=None):
    """chain_tc on a template rectangle (woft_chain_tc_window): flow (2, H, W) etc. are the planes of the
    rectangle with origin = (y0, x0) in a frame of frame_hw = (frame_h, frame_w); tmask_u8 is the CROPPED mask (mask_hw >= (H, W),
    default the grid's size).  dst (window coordinates), w and hist are chain_tc's bytes; ok is additionally 0 where the landing
    leaves the frame (the selection kernels' rule in frame coordinates)."""
    return _chain_tc("chain_tc_window", flow, cost, vis, sel, tmask_u8, None, vis_thr, (origin, frame_hw), want_w, mask_hw, out)


def chain_tc_multi(flow, cost, vis, sel, tbits, n_targets, vis_thr, want_w=True, mask_hw=None, out=None):
    """chain_tc for n_targets template masks at once (woft_chain_tc_multi) -> (dst (2, n), w (1, n) | None,
    ok (1, n), hist (n_targets, 130) int32).  tbits: the masks as one bit plane, an int32 device tensor of mask_hw = (mh, mw) >=
    (H, W) elements (default the grid's size), bit t set where the pixel lies in target t's mask.  dst, w, ok: chain_tc's bytes;
    hist[t]: chain_tc's for a uint8 mask equal to bit t.  out: the tuple of an earlier call at this size, reused (its hist may
    be a view into a larger result block)."""
    return _chain_tc("chain_tc_multi", flow, cost, vis, sel, tbits, n_targets, vis_thr, None, want_w, mask_hw, out)


def chain_tc_multi_window(flow, cost, vis, sel, tbits, n_targets, vis_thr, origin, frame_hw, want_w=True, mask_hw=None, out=None):
    """chain_tc_multi on a template rectangle (woft_chain_tc_multi_window): the planes are those of the
    rectangle with origin = (y0, x0) in a frame of frame_hw = (frame_h, frame_w); tbits is the bit plane CROPPED to the rectangle
    (mask_hw >= (H, W), default the grid's size).  dst (window coordinates), w and hist are chain_tc_multi's bytes; ok is
    additionally 0 where the landing leaves the frame: dst, w, ok are chain_tc_window's bytes, hist[t] its histogram for bit t."""
    return _chain_tc("chain_tc_multi_window", flow, cost, vis, sel, tbits, n_targets, vis_thr, (origin, frame_hw), want_w, mask_hw,
                     out)


def coords_update(coords, delta, ld_delta, wf, flow4=None, flow_cat=None, ld_cat=0):
    check(_lib.load().woft_coords_update(ptr(coords), ptr(delta), ld_delta, wf, coords.shape[0], ptr(flow4),
                                         ptr(flow_cat), ld_cat, stream_ptr()), "woft_coords_update")


def wh_needed(pts, count, n_max, top, left, hf, wf, index, bitmap, dyn_index, n_needed=None):
    """dyn_index[j] = index[j] where the weight-head window of 1/8-res pixel index[j] is needed by one of the (count) points
    pts (n_max, 2) = (x, y) image coordinates, else -1 (woft_wh_needed)."""
    check(_lib.load().woft_wh_needed(ptr(pts), ptr(count), n_max, top, left, hf, wf, ptr(index), index.numel(), ptr(bitmap),
                                     ptr(dyn_index), ptr(n_needed), stream_ptr()), "woft_wh_needed")


def colsum(f, n_pix, c, ws, total):
    """total[0..c) = fp64 column sums of the (n_pix, c) fp32 rows f; ws: (n_part, c) fp64 partial sums (woft_colsum)."""
    check(_lib.load().woft_colsum(ptr(f), n_pix, c, ptr(ws), ws.shape[0], ptr(total), stream_ptr()), "woft_colsum")


def wh_pack(lookup, f1, f2_total, alpha, nwin, mean, x8=None):
    """The weight head's mean-response channel mean[p] = alpha * <f1[p], f2_total> and, with x8, the (p, nwin, nwin, 8) input
    patches [4 lookup levels | mean] of its first conv (woft_wh_pack)."""
    check(_lib.load().woft_wh_pack(ptr(lookup.t), lookup.cs, ptr(f1.t), f1.c, ptr(f2_total), alpha, f1.n_pix, nwin, ptr(mean),
                                   ptr(x8.t) if x8 is not None else None, stream_ptr()), "woft_wh_pack")


def wh_conv0(lookup, mean, n_win, nwin, wt, bias, out, index=None):
    """The weight head's first conv + ReLU straight from the lookup buffer, on n_win windows (those of the source pixels listed
    in `index`, else all) (woft_wh_conv0)."""
    check(_lib.load().woft_wh_conv0(ptr(lookup.t), lookup.cs, ptr(mean), n_win, nwin, ptr(wt), ptr(bias), ptr(out.t), ptr(index),
                                    stream_ptr()), "woft_wh_conv0")


def wh_reduce(act, nwin2, w, bias, n_pix, out):
    """out[p] = bias + mean over the nwin2 window positions of <w, act[p][t]>: closing 1x1 conv + window mean (woft_wh_reduce)."""
    check(_lib.load().woft_wh_reduce(ptr(act.t), act.cs, nwin2, ptr(w), bias, n_pix, ptr(out), stream_ptr()), "woft_wh_reduce")


def copy_params(p):
    """A copy of a ctypes parameter struct that shares what the original carries besides its fields (_keep: the tensors its
    pointers refer to stay alive with the copy too)."""
    q = type(p).from_buffer_copy(p)
    q.__dict__.update(p.__dict__)
    return q


def warp_features(f, coords, out):
    """out[p, :f.c] = bilinear_sampler(f, coords[p]) for the out.n_pix pixels (woft_warp_features; grid_sample, align_corners=True,
    zero padding: utils/utils.py:59-73)."""
    check(_lib.load().woft_warp_features(ptr(f.t), f.h, f.w, f.c, f.cs, ptr(coords), out.n_pix, ptr(out.t), out.cs,
                                         stream_ptr()), "woft_warp_features")


def convex_upsample(coords, wlow, mask, hf, wf, crop, h, w, flow_up=None, dst=None, wout=None, do_sigmoid=False):
    check(_lib.load().woft_convex_upsample(ptr(coords), ptr(wlow), ptr(mask), mask.shape[1], hf, wf, crop[0], crop[1],
                                           h, w, ptr(flow_up), ptr(dst), ptr(wout), int(do_sigmoid), stream_ptr()),
          "woft_convex_upsample")


def convex_weights_at(pts, count, n_max, wlow, mask, hf, wf, crop, wsel, do_sigmoid=False):
    """wsel[i] = the weight convex_upsample would write at pixel pts[i] = (x, y), i < count (woft_convex_weights_at)."""
    check(_lib.load().woft_convex_weights_at(ptr(pts), ptr(count), n_max, ptr(wlow), ptr(mask), mask.shape[1], hf, wf,
                                             crop[0], crop[1], int(do_sigmoid), ptr(wsel), stream_ptr()),
          "woft_convex_weights_at")


# ---- training of the weight head (csrc/wh_train.hip) ----
WH_TRAIN_CHUNK = 16                     # WOFT_WH_TRAIN_CHUNK: windows per partial sum of the parameter gradients
WH_TRAIN_MAX_WIN = 9 * 2048             # WOFT_WH_TRAIN_MAX_WIN


def convex_weights_at_bwd(pts, count, n_max, g_wsel, wlow, mask, hf, wf, crop, g_wlow, index=None, do_sigmoid=False):
    """g_wlow (hf * wf floats, zeroed first) = the gradient of convex_weights_at's wsel with respect to wlow, at the cells listed
    in `index` (int32, None = every cell): woft_convex_weights_at_bwd."""
    assert _f32c(g_wsel) and g_wsel.numel() >= n_max and _f32c(g_wlow) and g_wlow.numel() == hf * wf
    n_win = hf * wf if index is None else index.numel()
    check(_lib.load().woft_convex_weights_at_bwd(ptr(pts), ptr(count), n_max, ptr(g_wsel), ptr(wlow), ptr(mask), mask.shape[1],
                                                 hf, wf, crop[0], crop[1], int(do_sigmoid), ptr(index), n_win, ptr(g_wlow),
                                                 stream_ptr()), "woft_convex_weights_at_bwd")


def wh_reduce_bwd(act, w6, g_wlow, index, n_win, g_act, ws, g_w6, g_b6):
    """Backward of the closing 1x1 conv + window mean on n_win windows of (n_win, 81, 128) activations: g_act, g_w6 (128),
    g_b6 (1); ws: at least ceil(n_win / WH_TRAIN_CHUNK) * 129 doubles (woft_wh_reduce_bwd)."""
    assert _f32c(act) and _f32c(g_act) and act.numel() >= n_win * 81 * 128 and g_act.numel() >= n_win * 81 * 128
    assert ws.dtype == torch.float64 and ws.numel() >= -(-n_win // WH_TRAIN_CHUNK) * 129
    assert _f32c(w6) and w6.numel() >= 128 and _f32c(g_w6) and g_w6.numel() >= 128 and _f32c(g_b6)
    assert index is None or (index.dtype == torch.int32 and index.numel() >= n_win)
    check(_lib.load().woft_wh_reduce_bwd(ptr(act), ptr(w6), ptr(g_wlow), ptr(index), n_win, ptr(g_act), ptr(ws), ptr(g_w6),
                                         ptr(g_b6), stream_ptr()), "woft_wh_reduce_bwd")


def wh_train_conv(x, cin, wt, n_win, y, bias=None, gate=None):
    """One 3x3 layer cin -> 128 on n_win 9x9 windows, exact fp32 (woft_wh_train_conv): x (n_win, 81, cin), wt (9, cin, 128),
    y (n_win, 81, 128); with bias: relu(conv + bias); with gate (n_win, 81, 128): conv where gate > 0, else 0."""
    assert _f32c(x) and x.numel() >= n_win * 81 * cin and _f32c(wt, 9, cin, 128) and _f32c(y) and y.numel() >= n_win * 81 * 128
    assert bias is None or (_f32c(bias) and bias.numel() == 128)
    assert gate is None or (_f32c(gate) and gate.numel() >= n_win * 81 * 128)
    check(_lib.load().woft_wh_train_conv(ptr(x), cin, ptr(wt), ptr(bias), ptr(gate), n_win, ptr(y), stream_ptr()),
          "woft_wh_train_conv")


def wh_wgrad_ws_floats(n_win, cin):
    return int(_lib.load().woft_wh_wgrad_ws_bytes(n_win, cin)) // 4


def wh_wgrad(gy, x, cin, n_win, ws, gw, gb):
    """Parameter gradient of a 3x3 layer cin -> 128 on n_win windows (woft_wh_wgrad): gy (n_win, 81, 128), x (n_win, 81, cin) ->
    gw (128, cin_out, 3, 3) with cin_out = gw.shape[1] <= cin, gb (128); ws: wh_wgrad_ws_floats(n_win, cin) floats."""
    assert _f32c(gy) and gy.numel() >= n_win * 81 * 128 and _f32c(x) and x.numel() >= n_win * 81 * cin
    assert _f32c(gw) and gw.shape[0] == 128 and tuple(gw.shape[2:]) == (3, 3) and _f32c(gb, 128)
    assert _f32c(ws) and ws.numel() >= wh_wgrad_ws_floats(n_win, cin)
    check(_lib.load().woft_wh_wgrad(ptr(gy), ptr(x), cin, gw.shape[1], n_win, ptr(ws), ptr(gw), ptr(gb), stream_ptr()),
          "woft_wh_wgrad")


# ---- training of the mask head (csrc/mh_train.hip) ----
MH_TRAIN_TILE = 32                      # WOFT_MH_TRAIN_TILE: positions of a map row per tile
MH_TRAIN_CHUNK = 16                     # WOFT_MH_TRAIN_CHUNK: tiles per partial sum of a weight gradient
MH_REDUCE_CHUNK = 256                   # WOFT_MH_REDUCE_CHUNK: pixels per partial sum of the closing conv's gradient


def _mh_map(t, n_pix, c):
    """A map of the training kernels: (rows >= n_pix, channel stride >= c) fp32, contiguous, on the device."""
    return _f32c(t) and t.dim() == 2 and t.shape[0] >= n_pix and t.shape[1] >= c


def _mh_sources(x0, x1, cin, n_pix):
    """-> the two-source arguments (x0, cs0, x1, cs1, c_split) of an input map of cin channels: x0 alone, or [x0 | x1] with
    cin / 2 channels each (the first layer's [fmap1 | warped fmap2])."""
    c_split = cin if x1 is None else cin // 2
    assert _mh_map(x0, n_pix, c_split) and (x1 is None or _mh_map(x1, n_pix, cin - c_split))
    return ptr(x0), x0.shape[1], ptr(x1), (0 if x1 is None else x1.shape[1]), c_split


def mh_train_conv(x0, x1, wt, hf, wf, y, bias=None, gate=None):
    """One 3x3 layer over the hf x wf map, zero padding, exact fp32 (woft_mh_train_conv): wt (9, cin, cout), input map x0 (or
    [x0 | x1], half of cin each), y a map of cout channels; with bias: relu(conv + bias); with gate (a map of cout channels): conv
    where gate > 0, else 0."""
    cin, cout = int(wt.shape[1]), int(wt.shape[2])
    P = hf * wf
    assert _f32c(wt, 9, cin, cout) and _mh_map(y, P, cout)
    assert bias is None or _f32c(bias, cout)
    assert gate is None or _mh_map(gate, P, cout)
    check(_lib.load().woft_mh_train_conv(*_mh_sources(x0, x1, cin, P), cin, ptr(wt), cout, ptr(bias), ptr(gate),
                                         0 if gate is None else gate.shape[1], hf, wf, ptr(y), y.shape[1], stream_ptr()),
          "woft_mh_train_conv")


def mh_wgrad_ws_floats(hf, wf, cin, cout):
    return int(_lib.load().woft_mh_wgrad_ws_bytes(hf, wf, cin, cout)) // 4


def mh_wgrad(gy, x0, x1, hf, wf, ws, gw, gb):
    """Parameter gradient of such a layer (woft_mh_wgrad): gy a map of cout channels, the input map x0 (or [x0 | x1]) -> gw
    (cout, cin, 3, 3), gb (cout); ws: mh_wgrad_ws_floats(hf, wf, cin, cout) floats."""
    cout, cin = int(gw.shape[0]), int(gw.shape[1])
    P = hf * wf
    assert _f32c(gw, cout, cin, 3, 3) and _f32c(gb, cout) and _mh_map(gy, P, cout)
    assert _f32c(ws) and ws.numel() >= mh_wgrad_ws_floats(hf, wf, cin, cout)
    check(_lib.load().woft_mh_wgrad(ptr(gy), gy.shape[1], cout, *_mh_sources(x0, x1, cin, P), cin, hf, wf, ptr(ws), ptr(gw),
                                    ptr(gb), stream_ptr()), "woft_mh_wgrad")


def mh_reduce_bwd(act, c, w, g_low, n_pix, g_act, ws, g_w, g_b):
    """Backward of the closing 1x1 conv on the n_pix pixels of a map of c channels: g_act (a map), g_w (c), g_b (1); ws: at least
    ceil(n_pix / MH_REDUCE_CHUNK) * 129 doubles (woft_mh_reduce_bwd)."""
    assert _mh_map(act, n_pix, c) and _mh_map(g_act, n_pix, c) and _f32c(g_low) and g_low.numel() >= n_pix
    assert ws.dtype == torch.float64 and ws.is_cuda and ws.numel() >= -(-n_pix // MH_REDUCE_CHUNK) * 129
    assert _f32c(w) and w.numel() >= c and _f32c(g_w) and g_w.numel() >= c and _f32c(g_b)
    check(_lib.load().woft_mh_reduce_bwd(ptr(act), act.shape[1], c, ptr(w), ptr(g_low), n_pix, ptr(g_act), g_act.shape[1], ptr(ws),
                                         ptr(g_w), ptr(g_b), stream_ptr()), "woft_mh_reduce_bwd")


# ---- dense adjoint of the convex upsampling (csrc/upsample_bwd.hip) ----
def convex_upsample_bwd_ws_floats(hf, wf):
    return int(_lib.load().woft_convex_upsample_bwd_ws_bytes(hf, wf)) // 4


def convex_upsample_bwd(g_up, mask, wlow, hf, wf, crop, h, w, ws, g_wlow, do_sigmoid=False):
    """g_wlow (hf * wf floats, written whole) = the gradient of convex_upsample's wout (h * w, cropped at `crop`) with respect to
    wlow for the upstream gradient g_up (h * w floats): woft_convex_upsample_bwd.  mask: (rows >= hf * wf, ld >= 576); wlow is
    read only with do_sigmoid (else it may be None); ws: convex_upsample_bwd_ws_floats(hf, wf) floats."""
    P = hf * wf
    assert _f32c(g_up) and g_up.numel() == h * w and _f32c(g_wlow) and g_wlow.numel() == P
    assert _f32c(mask) and mask.dim() == 2 and mask.shape[0] >= P and mask.shape[1] >= 576
    assert wlow is None or (_f32c(wlow) and wlow.numel() >= P)
    assert _f32c(ws) and ws.numel() >= convex_upsample_bwd_ws_floats(hf, wf)
    check(_lib.load().woft_convex_upsample_bwd(ptr(g_up), ptr(mask), mask.shape[1], ptr(wlow), hf, wf, crop[0], crop[1], h, w,
                                               int(do_sigmoid), ptr(ws), ptr(g_wlow), stream_ptr()), "woft_convex_upsample_bwd")


def upflow8(coords, wlow, hf, wf, crop, h, w, flow_up=None, dst=None, wout=None, do_sigmoid=False):
    check(_lib.load().woft_upflow8(ptr(coords), ptr(wlow), hf, wf, crop[0], crop[1], h, w, ptr(flow_up), ptr(dst),
                                   ptr(wout), int(do_sigmoid), stream_ptr()), "woft_upflow8")


def warp_perspective_u8(img, Hmat, out=None, valid=None, nearest=False):
    """img: (H,W,C) or (H,W) uint8 CUDA tensor; Hmat: 3x3 numpy (src -> dst).  dst(x) = src(H^-1 x)."""
    h, w = img.shape[:2]
    c = 1 if img.dim() == 2 else img.shape[2]
    arr = (C.c_double * 9)(*np.linalg.inv(np.asarray(Hmat, dtype=np.float64)).ravel().tolist())
    check(_lib.load().woft_warp_perspective_u8(ptr(img), h, w, c, arr, ptr(out), ptr(valid), int(nearest),
                                               stream_ptr()), "woft_warp_perspective_u8")


def _hinv9(Hmat):
    return (C.c_double * 9)(*np.linalg.inv(np.asarray(Hmat, dtype=np.float64)).ravel().tolist())


def _hsynth_occluders(occluders):
    """[(tex (ho, wo, 4) uint8 device tensor, H_occ 3x3 texture -> destination)] -> (ctypes array or None, n); the caller keeps
    `occluders` alive until the launch is enqueued."""
    n = len(occluders)
    if n == 0:
        return None, 0
    arr = (_lib.HSynthOccluder * n)()
    for k, (tex, H_occ) in enumerate(occluders):
        arr[k].tex, arr[k].ho, arr[k].wo = ptr(tex), tex.shape[0], tex.shape[1]
        arr[k].hinv[:] = np.linalg.inv(np.asarray(H_occ, dtype=np.float64)).ravel().tolist()
    return arr, n


def hsynth_render(base, Hmat, occluders, gain, bias, out_u8, out_f32=None, cover=None):
    """woft_hsynth_render: out_u8 (h, w, 3) = base (hs, ws, 3) seen through Hmat (base -> destination), times gain plus bias
    (3 floats each or None), under the occluders in order; out_f32 / cover as the header says.  Inversions in fp64 on the host."""
    hs, ws = base.shape[:2]
    h, w = out_u8.shape[:2]
    occ, n = _hsynth_occluders(occluders)
    g = None if gain is None else (C.c_float * 3)(*[float(v) for v in gain])
    b = None if bias is None else (C.c_float * 3)(*[float(v) for v in bias])
    check(_lib.load().woft_hsynth_render(ptr(base), hs, ws, _hinv9(Hmat), g, b, occ, n, ptr(out_u8), ptr(out_f32), ptr(cover),
                                         h, w, stream_ptr()), "woft_hsynth_render")


def hsynth_render_bg(base, Hmat, occluders, gain, bias, bg, Hbg, out_u8, out_f32=None, cover=None, plane=None):
    """woft_hsynth_render_bg: hsynth_render with the background bg ((hb, wb, 3) uint8) seen through Hbg (background -> destination)
    behind the plane; plane (h, w) float32 or None = the plane's coverage."""
    hs, ws = base.shape[:2]
    h, w = out_u8.shape[:2]
    occ, n = _hsynth_occluders(occluders)
    g = None if gain is None else (C.c_float * 3)(*[float(v) for v in gain])
    b = None if bias is None else (C.c_float * 3)(*[float(v) for v in bias])
    check(_lib.load().woft_hsynth_render_bg(ptr(base), hs, ws, _hinv9(Hmat), g, b, occ, n, ptr(bg), bg.shape[0], bg.shape[1],
                                            _hinv9(Hbg), ptr(out_u8), ptr(out_f32), ptr(cover), ptr(plane), h, w, stream_ptr()),
          "woft_hsynth_render_bg")


def hsynth_augment(frame, taps, colour, noise_sigma, seed, out_u8, out_f32=None):
    """woft_hsynth_augment: frame (h, w, 3) float32 -> out_u8 (and out_f32) through the blur with `taps` (2 r + 1 float32 values,
    None or one value = no blur), the affine colour map `colour` (12 float32 values: M row-major, then the offset; None =
    identity), noise of noise_sigma from the 32-bit seed.  out_f32 may be `frame` itself when there is no blur."""
    assert _f32c(frame) and frame.dim() == 3 and frame.shape[2] == 3
    h, w = frame.shape[:2]
    radius = 0 if taps is None else (len(taps) - 1) // 2
    t = None if radius == 0 else (C.c_float * len(taps))(*[float(v) for v in taps])
    m = None if colour is None else (C.c_float * 12)(*[float(v) for v in colour])
    check(_lib.load().woft_hsynth_augment(ptr(frame), h, w, t, radius, m, float(noise_sigma), int(seed) & 0xFFFFFFFF, ptr(out_u8),
                                          ptr(out_f32), stream_ptr()), "woft_hsynth_augment")


def hsynth_labels(src_hw, Hmat, occluders, out_hw, lo, hi, flow, visible, valid):
    """woft_hsynth_labels: flow (2, hs, ws) float32, visible (hs, ws) float32, valid (hs, ws) bool / uint8 of the template pixels
    under Hmat (base -> destination) and the occluders."""
    occ, n = _hsynth_occluders(occluders)
    hf = (C.c_double * 9)(*np.asarray(Hmat, dtype=np.float64).ravel().tolist())
    check(_lib.load().woft_hsynth_labels(src_hw[0], src_hw[1], hf, occ, n, out_hw[0], out_hw[1], lo, hi, ptr(flow), ptr(visible),
                                         ptr(valid), stream_ptr()), "woft_hsynth_labels")


def warp_perspective_window_u8(img, Hmat, rect, out=None, valid=None, nearest=False):
    """The rectangle rect = (y0, x0, rows, cols) of warp_perspective_u8(img, Hmat, ...) into contiguous (rows, cols[, C]) `out`
    and (rows, cols) `valid`: the same bytes as the full-frame call gives those destination pixels, for the window's work."""
    h, w = img.shape[:2]
    c = 1 if img.dim() == 2 else img.shape[2]
    y0, x0, rows, cols = (int(v) for v in rect)
    assert out is None or out.numel() == rows * cols * c
    assert valid is None or valid.numel() == rows * cols
    check(_lib.load().woft_warp_perspective_window_u8(ptr(img), h, w, c, _hinv9(Hmat), y0, x0, rows, cols, ptr(out), ptr(valid),
                                                      int(nearest), stream_ptr()), "woft_warp_perspective_window_u8")


def crop_u8(img, rect, out=None):
    """img[y0:y0 + rows, x0:x0 + cols] of a packed (H, W[, C]) uint8 tensor as a contiguous tensor (woft_crop_u8)."""
    h, w = img.shape[:2]
    c = 1 if img.dim() == 2 else img.shape[2]
    y0, x0, rows, cols = (int(v) for v in rect)
    if out is None:
        out = torch.empty((rows, cols) + tuple(img.shape[2:]), dtype=torch.uint8, device=img.device)
    assert out.numel() == rows * cols * c and out.is_contiguous() and img.is_contiguous()
    check(_lib.load().woft_crop_u8(ptr(img), h, w, c, y0, x0, rows, cols, ptr(out), stream_ptr()), "woft_crop_u8")
    return out


_BBOX_WS = {}


def mask_bbox_ws(device=None):
    """Scratch of woft_mask_bbox, zeroed once (every call leaves it zeroed); one per device and stream, like hfit_ws."""
    dev = torch.device(device or DEV)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), stream_ptr())
    if key not in _BBOX_WS:
        _BBOX_WS[key] = torch.zeros(int(_lib.load().woft_mask_bbox_ws_bytes()), dtype=torch.uint8, device=dev)
    return _BBOX_WS[key]


def mask_bbox(mask, bbox=None, Hmat=None, warped=None, ws=None):
    """{rmin, rmax, cmin, cmax, any} (5 int32 on the device) of the non-zero pixels of a (H, W) uint8 mask -- or, with Hmat, of
    warp_perspective_u8(mask, Hmat, nearest=True), which `warped` (optional) receives in the same launch."""
    h, w = mask.shape
    if bbox is None:
        bbox = torch.empty(5, dtype=torch.int32, device=mask.device)
    assert mask.is_contiguous() and (warped is None or (warped.is_contiguous() and warped.numel() == h * w))
    ws = ws if ws is not None else mask_bbox_ws(mask.device)
    check(_lib.load().woft_mask_bbox(ptr(mask), h, w, None if Hmat is None else _hinv9(Hmat), ptr(warped), ptr(ws), ptr(bbox),
                                     stream_ptr()), "woft_mask_bbox")
    return bbox


def mask_bbox_multi_ws(n_targets, device=None):
    """Scratch of woft_mask_bbox_multi for n_targets, zeroed once (every call leaves it zeroed); one per device, stream and count."""
    dev = torch.device(device or DEV)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), stream_ptr(), int(n_targets))
    if key not in _BBOX_WS:
        need = int(_lib.load().woft_mask_bbox_multi_ws_bytes(int(n_targets)))
        if need < 0:
            raise _lib.WoftHipError(f"woft_mask_bbox_multi_ws_bytes({n_targets}) rejected its argument")
        _BBOX_WS[key] = torch.zeros(need, dtype=torch.uint8, device=dev)
    return _BBOX_WS[key]


def mask_bbox_multi(tbits, n_targets, Hmats, bbox=None, ws=None):
    """mask_bbox(mask_t, Hmat=Hmats[t]) for the n_targets masks of a bit plane in ONE launch (woft_mask_bbox_multi; DESIGN.md
    section 28) -> bbox (n_targets, 5) int32 on the device, row t = {rmin, rmax, cmin, cmax, any} of mask t carried by Hmats[t]
    (3 x 3, mask -> frame; inverted in fp64 on the host, as mask_bbox does).  Hmats[t] None: target t is skipped, its row is zeros.
    tbits: the (H, W) int32 bit plane of chain_tc_multi."""
    assert tbits.dim() == 2
    h, w = tbits.shape
    _check_tbits(tbits, h, w, n_targets)
    if len(Hmats) != n_targets:
        raise ValueError(f"mask_bbox_multi: {n_targets} targets, {len(Hmats)} homographies")
    hinv, skip = (C.c_double * (9 * n_targets))(), 0
    for t, Hm in enumerate(Hmats):
        if Hm is None:
            skip |= 1 << t
        else:
            hinv[9 * t:9 * t + 9] = np.linalg.inv(np.asarray(Hm, dtype=np.float64)).ravel().tolist()
    if bbox is None:
        bbox = torch.empty(n_targets, 5, dtype=torch.int32, device=tbits.device)
    assert bbox.dtype == torch.int32 and bbox.is_contiguous() and bbox.numel() == 5 * n_targets
    ws = ws if ws is not None else mask_bbox_multi_ws(n_targets, tbits.device)
    check(_lib.load().woft_mask_bbox_multi(ptr(tbits), h, w, int(n_targets), hinv, skip, ptr(ws), ptr(bbox), stream_ptr()),
          "woft_mask_bbox_multi")
    return bbox


def resize_by_factor_u8(img, factor):
    """cv2.resize(img, None, fx=1/factor, fy=1/factor) (INTER_LINEAR geometry) on the device."""
    h, w = img.shape[:2]
    c = 1 if img.dim() == 2 else img.shape[2]
    ho, wo = int(round(h / factor)), int(round(w / factor))
    out = torch.empty((ho, wo) if img.dim() == 2 else (ho, wo, c), dtype=torch.uint8, device=img.device)
    check(_lib.load().woft_resize_linear_u8(ptr(img), h, w, c, ptr(out), ho, wo, float(factor), float(factor),
                                            stream_ptr()), "woft_resize_linear_u8")
    return out


def tc_select_ws(n):
    return torch.empty(int(_lib.load().woft_tc_select_ws_bytes(n)), dtype=torch.uint8, device=DEV)


def tc_select(dst, w, tmask_u8, pwmask_u8, h, wimg, check_dst, sobol_u, ws, pa, pb, wout, count, grid=None):
    """Mask + compact + Sobol-subsample correspondences on the device (see csrc/select.hip).  (h, wimg): size of the
    masks (the frame); grid = (gh, gw): size of the flow grid when it differs (padding_mode 'crop')."""
    n_draw = 0 if sobol_u is None else sobol_u.numel()
    gh, gw = grid or (h, wimg)
    assert dst.numel() == 2 * gh * gw and tmask_u8.numel() == h * wimg and (w is None or w.numel() == gh * gw)
    check(_lib.load().woft_tc_select(ptr(dst), ptr(w), ptr(tmask_u8), ptr(pwmask_u8), gh, gw, h, wimg, int(check_dst),
                                     ptr(sobol_u), n_draw, ptr(ws), ptr(pa), ptr(pb), ptr(wout), pa.shape[0],
                                     ptr(count), stream_ptr()), "woft_tc_select")


def tc_flags(dst, tmask_u8, pwmask_u8, h, wimg, check_dst, grid=None, out=None):
    """The keep rule of tc_select alone -> bool tensor (gh*gw,) (woft_tc_flags)."""
    gh, gw = grid or (h, wimg)
    assert tmask_u8.numel() == h * wimg and (dst is None or dst.numel() == 2 * gh * gw)
    flags = out if out is not None else torch.empty(gh * gw, dtype=torch.uint8, device=tmask_u8.device)
    check(_lib.load().woft_tc_flags(ptr(dst), ptr(tmask_u8), ptr(pwmask_u8), gh, gw, h, wimg, int(check_dst),
                                    ptr(flags), stream_ptr()), "woft_tc_flags")
    return flags.view(torch.bool)


VIS_MODES = {"gate": 1, "weight": 2}


def tc_select_vis(dst, w, tmask_u8, pwmask_u8, h, wimg, check_dst, sobol_u, vis, vis_mode, vis_thr, ws, pa, pb, wout, count,
                  grid=None):
    """tc_select with the visibility probability vis (gh*gw floats; woft_tc_select_vis).  vis_mode 'gate': survivors also need
    vis > vis_thr; 'weight': wout = w * vis (vis alone when w is None); None / 0: tc_select."""
    n_draw = 0 if sobol_u is None else sobol_u.numel()
    gh, gw = grid or (h, wimg)
    assert dst.numel() == 2 * gh * gw and tmask_u8.numel() == h * wimg and (w is None or w.numel() == gh * gw)
    assert vis is None or (vis.numel() == gh * gw and vis.dtype == torch.float32)
    mode = VIS_MODES[vis_mode] if isinstance(vis_mode, str) else int(vis_mode or 0)
    check(_lib.load().woft_tc_select_vis(ptr(dst), ptr(w), ptr(tmask_u8), ptr(pwmask_u8), gh, gw, h, wimg, int(check_dst),
                                         ptr(sobol_u), n_draw, ptr(vis), mode, float(vis_thr), ptr(ws), ptr(pa), ptr(pb),
                                         ptr(wout), pa.shape[0], ptr(count), stream_ptr()), "woft_tc_select_vis")


def tc_select_multi_ws(n, n_targets):
    need = int(_lib.load().woft_tc_select_multi_ws_bytes(int(n), int(n_targets)))
    if need < 0:
        raise _lib.WoftHipError(f"woft_tc_select_multi_ws_bytes({n}, {n_targets}) rejected its arguments")
    return torch.empty(need, dtype=torch.uint8, device=DEV)


def tc_select_multi(dst, w, tbits, n_targets, h, wimg, check_dst, sobol_u, vis, vis_mode, vis_thr, ws, pa, pb, wout, count,
                    grid=None):
    """tc_select_vis for n_targets template masks at once (woft_tc_select_multi).  tbits: the bit plane of
    chain_tc_multi (int32, h * wimg elements); pa, pb (n_targets, cap, 2), wout (n_targets, cap) or None, count (2, n_targets)
    int32: row 0 the selected counts (the `counts` of hfit_batched), row 1 the kept ones.  The first count[0, t] rows of target
    t's slices are what tc_select_vis writes for a uint8 mask equal to bit t and no pwmask."""
    n_draw = 0 if sobol_u is None else sobol_u.numel()
    gh, gw = grid or (h, wimg)
    _check_tbits(tbits, h, wimg, n_targets)
    assert dst.numel() == 2 * gh * gw and (w is None or w.numel() == gh * gw)
    assert vis is None or (vis.numel() == gh * gw and vis.dtype == torch.float32)
    cap = pa.shape[1]
    assert tuple(pa.shape) == tuple(pb.shape) == (n_targets, cap, 2) and pa.is_contiguous() and pb.is_contiguous()
    assert wout is None or (tuple(wout.shape) == (n_targets, cap) and wout.is_contiguous())
    assert count.dtype == torch.int32 and count.is_contiguous() and count.numel() == 2 * n_targets
    mode = VIS_MODES[vis_mode] if isinstance(vis_mode, str) else int(vis_mode or 0)
    check(_lib.load().woft_tc_select_multi(ptr(dst), ptr(w), ptr(tbits), gh, gw, h, wimg, int(n_targets), int(check_dst),
                                           ptr(sobol_u), n_draw, ptr(vis), mode, float(vis_thr), ptr(ws), ptr(pa), ptr(pb),
                                           ptr(wout), cap, ptr(count), stream_ptr()), "woft_tc_select_multi")


def tc_flags_vis(dst, tmask_u8, pwmask_u8, h, wimg, check_dst, vis, vis_mode, vis_thr, grid=None, out=None):
    """The keep rule of tc_select_vis alone -> bool tensor (gh*gw,) (woft_tc_flags_vis): gated in mode 'gate' only."""
    gh, gw = grid or (h, wimg)
    assert tmask_u8.numel() == h * wimg and (dst is None or dst.numel() == 2 * gh * gw)
    assert vis is None or (vis.numel() == gh * gw and vis.dtype == torch.float32)
    mode = VIS_MODES[vis_mode] if isinstance(vis_mode, str) else int(vis_mode or 0)
    flags = out if out is not None else torch.empty(gh * gw, dtype=torch.uint8, device=tmask_u8.device)
    check(_lib.load().woft_tc_flags_vis(ptr(dst), ptr(tmask_u8), ptr(pwmask_u8), gh, gw, h, wimg, int(check_dst), ptr(vis),
                                        mode, float(vis_thr), ptr(flags), stream_ptr()), "woft_tc_flags_vis")
    return flags.view(torch.bool)


def _stream_scratch(cache, need, device):
    """`need` bytes of estimator scratch out of `cache`: one buffer per device AND stream (its use is ordered by the stream it was
    first used on -- two trackers on two streams of one process must not share it), reused, grown on demand."""
    dev = torch.device(device or DEV)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(), stream_ptr())
    if key not in cache or cache[key].numel() < need:
        cache[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    return cache[key]


_HFIT_WS, _RANSAC_WS, _TRS_WS = {}, {}, {}


def hfit_ws(device=None):
    """Scratch of the streaming fit (woft_hfit_ws_bytes), one per device and stream, reused (stream-ordered)."""
    return _stream_scratch(_HFIT_WS, int(_lib.load().woft_hfit_ws_bytes()), device)


HFIT_SINGLE_MAX = 2048


def hfit(pa, pb, w, Hout, status, count=None, reweight=0, huber_k=1.0, n_irls=0, ws=None):
    n = pa.shape[0]
    if ws is None and n > HFIT_SINGLE_MAX:
        ws = hfit_ws(pa.device)
    check(_lib.load().woft_hfit(ptr(pa), ptr(pb), ptr(w), n, ptr(count), reweight, float(huber_k), n_irls,
                                ptr(ws), ptr(Hout), ptr(status), stream_ptr()), "woft_hfit")


HFIT_BATCH_MAX = 65535


def hfit_batched(pa, pb, w, Hout, status, counts=None, reweight=0, huber_k=1.0, n_irls=0):
    """B independent fits of N <= HFIT_SINGLE_MAX correspondences each in one launch (woft_hfit_batched): pa, pb (B, N, 2),
    w (B, N) or None, Hout (B, 9) or (B, 3, 3), status (B,) int32, counts (B,) int32 or None -- all contiguous, fp32, on one
    device.  Element b gets the bits of hfit() on element b alone.  More than HFIT_BATCH_MAX elements: one launch per
    HFIT_BATCH_MAX of them."""
    B, n = pa.shape[0], pa.shape[1]
    fn = _lib.load().woft_hfit_batched
    for lo in range(0, B, HFIT_BATCH_MAX):
        hi = min(B, lo + HFIT_BATCH_MAX)
        check(fn(ptr(pa[lo:hi]), ptr(pb[lo:hi]), ptr(w[lo:hi]) if w is not None else None, hi - lo, n,
                 ptr(counts[lo:hi]) if counts is not None else None, reweight, float(huber_k), n_irls, ptr(Hout[lo:hi]),
                 ptr(status[lo:hi]), stream_ptr()), "woft_hfit_batched")


def hfit_batched_bwd(pa, pb, w, gH, gpa, gpb, gw, status=None, counts=None):
    """Backward of the plain weighted fit (woft_hfit_batched_bwd; reweight 0, N <= HFIT_SINGLE_MAX) in one launch, one
    workgroup per element: pa, pb (B, N, 2), w (B, N) or None, gH (B, 9) or (B, 3, 3) the gradient with respect to the fit's
    output; gpa, gpb (B, N, 2), gw (B, N) receive the gradients, any of them None = not wanted (gw needs w); status (B,) int32
    or None, counts (B,) int32 or None -- all contiguous, fp32, on one device.  An element whose fit fails gets zeros.  More than
    HFIT_BATCH_MAX elements: one launch per HFIT_BATCH_MAX of them."""
    B, n = pa.shape[0], pa.shape[1]
    fn = _lib.load().woft_hfit_batched_bwd
    sl = lambda t, lo, hi: ptr(t[lo:hi]) if t is not None else None
    for lo in range(0, B, HFIT_BATCH_MAX):
        hi = min(B, lo + HFIT_BATCH_MAX)
        check(fn(ptr(pa[lo:hi]), ptr(pb[lo:hi]), sl(w, lo, hi), hi - lo, n, sl(counts, lo, hi), ptr(gH[lo:hi]), sl(gpa, lo, hi),
                 sl(gpb, lo, hi), sl(gw, lo, hi), sl(status, lo, hi), stream_ptr()), "woft_hfit_batched_bwd")


def hfit_step(pa, pb, w, rew, first, res, Hout, status, ws=None):
    """One re-weighted solve with externally supplied row re-weights; residuals of its solution -> res."""
    ws = ws if ws is not None else hfit_ws(pa.device)
    check(_lib.load().woft_hfit_step(ptr(pa), ptr(pb), ptr(w), pa.shape[0], ptr(rew), int(bool(first)), ptr(ws),
                                     ptr(res), ptr(Hout), ptr(status), stream_ptr()), "woft_hfit_step")


def ransac_ws(n_max, max_iters, device=None):
    """Scratch of woft_ransac (woft_ransac_ws_bytes(n_max, max_iters)), one per device and stream like hfit_ws, grown on demand."""
    need = int(_lib.load().woft_ransac_ws_bytes(int(n_max), int(max_iters)))
    if need < 0:
        raise _lib.WoftHipError(f"woft_ransac_ws_bytes({n_max}, {max_iters}) rejected its arguments")
    return _stream_scratch(_RANSAC_WS, need, device)


def ransac(pa, pb, Hout, status, count=None, max_iters=10000, thr=1.4142, conf=0.995, seed=0, refine=True, info=None,
           inlier_mask=None, ws=None):
    """RANSAC homography pa -> pb (csrc/ransac.hip): Hout 9 floats, status 1 int32, info 3 int32 (inliers, best k, iterations) and
    inlier_mask uint8 [n_max] optional; n = min(count[0], n_max) when count is given."""
    n = pa.shape[0]
    ws = ws if ws is not None else ransac_ws(n, max_iters, pa.device)
    check(_lib.load().woft_ransac(ptr(pa), ptr(pb), n, ptr(count), int(max_iters), float(thr), float(conf),
                                  int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(refine)), ptr(ws), ptr(Hout), ptr(status), ptr(info),
                                  ptr(inlier_mask), stream_ptr()), "woft_ransac")


def trs_ws(n_max, max_iters, device=None):
    """Scratch of woft_trs (woft_trs_ws_bytes(n_max, max_iters)), one per device and stream like ransac_ws, grown on demand."""
    need = int(_lib.load().woft_trs_ws_bytes(int(n_max), int(max_iters)))
    if need < 0:
        raise _lib.WoftHipError(f"woft_trs_ws_bytes({n_max}, {max_iters}) rejected its arguments")
    return _stream_scratch(_TRS_WS, need, device)


def trs(pa, pb, Hout, status, count=None, max_iters=10000, thr=3.0, conf=0.999, seed=0, refine=True, info=None,
        inlier_mask=None, ws=None):
    """RANSAC similarity pa -> pb (csrc/trs.hip): Hout 9 floats, status 1 int32, info 3 int32 (inliers, best k, iterations) and
    inlier_mask uint8 [n_max] optional; n = min(count[0], n_max) when count is given."""
    n = pa.shape[0]
    ws = ws if ws is not None else trs_ws(n, max_iters, pa.device)
    check(_lib.load().woft_trs(ptr(pa), ptr(pb), n, ptr(count), int(max_iters), float(thr), float(conf),
                               int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(refine)), ptr(ws), ptr(Hout), ptr(status), ptr(info),
                               ptr(inlier_mask), stream_ptr()), "woft_trs")


def inlier_frac(pa, pb, Hm, frac, thr=5.0, count=None):
    check(_lib.load().woft_inlier_frac(ptr(pa), ptr(pb), pa.shape[0], ptr(count), ptr(Hm), float(thr), ptr(frac),
                                       stream_ptr()), "woft_inlier_frac")


def inlier_frac_batched(pa, pb, Hm, frac, thr=5.0, counts=None):
    """B inlier tests in one launch (woft_inlier_frac_batched): pa, pb (B, N, 2), Hm (B, 9) or (B, 3, 3), frac (B,), counts (B,)
    int32 or None -- contiguous, on one device.  Element b gets the bits of inlier_frac() on element b alone."""
    B, n = pa.shape[0], pa.shape[1]
    assert tuple(pb.shape) == (B, n, 2) and pa.is_contiguous() and pb.is_contiguous() and Hm.is_contiguous() and frac.is_contiguous()
    assert Hm.numel() == 9 * B and frac.numel() == B and (counts is None or (counts.dtype == torch.int32 and counts.numel() == B
                                                                              and counts.is_contiguous()))
    check(_lib.load().woft_inlier_frac_batched(ptr(pa), ptr(pb), B, n, ptr(counts), ptr(Hm), float(thr), ptr(frac), stream_ptr()),
          "woft_inlier_frac_batched")


_PHOTO_WS = {}
PHOTO_NACC, PHOTO_REC, PHOTO_MAX_ITERS, PHOTO_CHUNK = 68, 16, 64, 2048       # the WOFT_PHOTO_* constants of include/woft_hip.h
PHOTO_STATUS = ("CONVERGED", "MAX_ITERS", "TOO_FEW", "SINGULAR", "NONFINITE")      # enum woft_photo_status


def photo_ws(box, stride, device=None):
    """Scratch of woft_photo_eval / woft_photo_refine for the inclusive box (x0, y0, x1, y1), one per device and stream like
    hfit_ws, grown on demand."""
    need = int(_lib.load().woft_photo_ws_bytes(box[2] - box[0] + 1, box[3] - box[1] + 1, int(stride)))
    if need < 0:
        raise _lib.WoftHipError(f"woft_photo_ws_bytes rejected box {tuple(box)!r}, stride {stride!r}")
    return _stream_scratch(_PHOTO_WS, need, device)


def _photo_images(tmpl, mask, weights, frame):
    for t, what in ((tmpl, "template"), (frame, "frame")):
        assert t.dtype in (torch.uint8, torch.float32) and t.dim() == 3 and t.shape[2] == 3 and t.is_contiguous(), what
    h, w = tmpl.shape[:2]
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (h, w) and mask.is_contiguous()
    assert weights is None or (_f32c(weights) and tuple(weights.shape) == (h, w))
    return (ptr(tmpl), int(tmpl.dtype == torch.float32), ptr(mask), h, w, ptr(weights), ptr(frame),
            int(frame.dtype == torch.float32), frame.shape[0], frame.shape[1])


def _photo_huber(huber_k):
    return -1.0 if huber_k is None else float(huber_k)


def photo_eval(tmpl, mask, weights, frame, box, stride, W, gain, bias, gain_bias, huber_k, out, ws=None):
    """woft_photo_eval: the normal equations of the photometric refinement at one state -> out (PHOTO_NACC float64 on the device):
    the upper triangle of G row-major, r, sum weight * rho, sum weight, n_valid.  W: 3x3 template -> frame pixels; bias in units
    of the three-channel sum."""
    ws = ws if ws is not None else photo_ws(box, stride, tmpl.device)
    assert out.dtype == torch.float64 and out.numel() >= PHOTO_NACC and out.is_contiguous()
    check(_lib.load().woft_photo_eval(*_photo_images(tmpl, mask, weights, frame), (C.c_int32 * 4)(*[int(v) for v in box]),
                                      int(stride), (C.c_double * 9)(*np.asarray(W, dtype=np.float64).ravel().tolist()),
                                      float(gain), float(bias), int(bool(gain_bias)), _photo_huber(huber_k), ptr(ws), ptr(out),
                                      stream_ptr()), "woft_photo_eval")


def photo_refine(tmpl, mask, weights, frame, box, stride, W0, iters, gain_bias, huber_k, n_need, eps, result, ws=None):
    """woft_photo_refine: iters + 1 (accumulate, step) launch pairs from W0 -> result (PHOTO_REC * (iters + 2) float64 on the
    device; layout in include/woft_hip.h)."""
    ws = ws if ws is not None else photo_ws(box, stride, tmpl.device)
    assert result.dtype == torch.float64 and result.numel() >= PHOTO_REC * (iters + 2) and result.is_contiguous()
    check(_lib.load().woft_photo_refine(*_photo_images(tmpl, mask, weights, frame), (C.c_int32 * 4)(*[int(v) for v in box]),
                                        int(stride), (C.c_double * 9)(*np.asarray(W0, dtype=np.float64).ravel().tolist()),
                                        int(iters), int(bool(gain_bias)), _photo_huber(huber_k), int(n_need), float(eps), ptr(ws),
                                        ptr(result), stream_ptr()), "woft_photo_refine")


PHOTO_STATUS_MULTI = PHOTO_STATUS + ("SKIPPED",)    # (WOFT_PHOTO_SKIPPED: an inactive target of the multi-target forms)


def photo_multi_partials(boxes, stride):
    """P_max of woft_photo_*_multi: the largest number of WOFT_PHOTO_CHUNK partials of any of the K inclusive boxes."""
    s = int(stride)
    return max(-(-(((int(b[2]) - int(b[0])) // s + 1) * ((int(b[3]) - int(b[1])) // s + 1)) // PHOTO_CHUNK) for b in boxes)


def photo_multi_ws(boxes, stride, device=None):
    """Scratch of woft_photo_eval_multi / woft_photo_refine_multi for K inclusive boxes, shared with the single forms' (one per
    device and stream, grown on demand)."""
    need = int(_lib.load().woft_photo_multi_ws_bytes(len(boxes), photo_multi_partials(boxes, stride)))
    if need < 0:
        raise _lib.WoftHipError(f"woft_photo_multi_ws_bytes rejected {len(boxes)} boxes, stride {stride!r}")
    return _stream_scratch(_PHOTO_WS, need, device)


def _photo_multi_args(tmpl, bits, weights, frame, boxes, W):
    K = len(boxes)
    for t, what in ((tmpl, "template"), (frame, "frame")):
        assert t.dtype in (torch.uint8, torch.float32) and t.dim() == 3 and t.shape[2] == 3 and t.is_contiguous(), what
    h, w = tmpl.shape[:2]
    assert bits.dtype == torch.int32 and tuple(bits.shape) == (h, w) and bits.is_contiguous()
    assert weights is None or (_f32c(weights) and tuple(weights.shape) == (h, w))
    W = np.asarray(W, dtype=np.float64).reshape(K, 9)
    return ((ptr(tmpl), int(tmpl.dtype == torch.float32), ptr(bits), h, w, ptr(weights), ptr(frame),
             int(frame.dtype == torch.float32), frame.shape[0], frame.shape[1], K,
             (C.c_int32 * (4 * K))(*[int(v) for b in boxes for v in b])), (C.c_double * (9 * K))(*W.ravel().tolist()))


def _i32s(values, K):
    assert len(values) == K
    return (C.c_int32 * K)(*[int(v) for v in values])


def photo_eval_multi(tmpl, bits, weights, frame, boxes, stride, W, gains, biases, active, gain_bias, huber_k, out, ws=None):
    """woft_photo_eval_multi: the normal equations of K targets of one template and one frame at K states -> out ((K, PHOTO_NACC)
    float64 on the device; row t as photo_eval writes it on target t's mask, untouched where active[t] is 0).  bits: the (h, w)
    int32 view of the targets' bit plane; boxes (K, 4), W (K, 3, 3), gains, biases, active (K) on the host."""
    K = len(boxes)
    ws = ws if ws is not None else photo_multi_ws(boxes, stride, tmpl.device)
    assert out.dtype == torch.float64 and out.numel() >= K * PHOTO_NACC and out.is_contiguous()
    head, Wc = _photo_multi_args(tmpl, bits, weights, frame, boxes, W)
    dbl = lambda v: (C.c_double * K)(*[float(x) for x in v])
    assert len(gains) == K and len(biases) == K
    check(_lib.load().woft_photo_eval_multi(*head, int(stride), Wc, dbl(gains), dbl(biases), _i32s(active, K), int(bool(gain_bias)),
                                            _photo_huber(huber_k), ptr(ws), ptr(out), stream_ptr()), "woft_photo_eval_multi")


def photo_refine_multi(tmpl, bits, weights, frame, boxes, stride, W0, n_need, active, iters, gain_bias, huber_k, eps, result,
                       ws=None):
    """woft_photo_refine_multi: iters + 1 (accumulate, step) launch pairs for K targets of one template and one frame -> result
    (K blocks of PHOTO_REC * (iters + 2) float64 on the device, each photo_refine's block of that target)."""
    K = len(boxes)
    ws = ws if ws is not None else photo_multi_ws(boxes, stride, tmpl.device)
    assert result.dtype == torch.float64 and result.numel() >= K * PHOTO_REC * (iters + 2) and result.is_contiguous()
    head, Wc = _photo_multi_args(tmpl, bits, weights, frame, boxes, W0)
    check(_lib.load().woft_photo_refine_multi(*head, int(stride), Wc, _i32s(n_need, K), _i32s(active, K), int(iters),
                                              int(bool(gain_bias)), _photo_huber(huber_k), float(eps), ptr(ws), ptr(result),
                                              stream_ptr()), "woft_photo_refine_multi")


PHOTO_WEIGHTS_MAX_RADIUS = 4                        # WOFT_PHOTO_WEIGHTS_MAX_RADIUS
PHOTO_WEIGHT_MODES = ("gate", "soft")               # woft_photo_weights' mode 0 / 1


def photo_weights(cost, vis, rect, template_hw, bits, n_targets, vis_thr, mode, radius, out_map, support):
    """woft_photo_weights: the fold planes cost, vis (fp32 device tensors of rows * cols elements) on rect = (ry, rx, rows, cols) of a
    template of template_hw = (h, w) -> out_map ((h, w) fp32, every entry written) and support (n_targets int32; None with
    n_targets = 0, and then bits may be None).  bits: the (h, w) int32 view of the targets' bit plane.  mode: 0 gate, 1 soft."""
    ry, rx, rows, cols = (int(v) for v in rect)
    h, w = (int(v) for v in template_hw)
    assert all(_f32c(t) and t.numel() == rows * cols for t in (cost, vis))
    assert _f32c(out_map, h, w)
    n_targets = int(n_targets)
    if n_targets > 0:
        assert bits.dtype == torch.int32 and tuple(bits.shape) == (h, w) and bits.is_contiguous() and bits.is_cuda
        assert support.dtype == torch.int32 and support.numel() >= n_targets and support.is_contiguous() and support.is_cuda
    check(_lib.load().woft_photo_weights(ptr(cost), ptr(vis), rows, cols, ry, rx, h, w, ptr(bits) if n_targets > 0 else None,
                                         n_targets, float(vis_thr), int(mode), int(radius), ptr(out_map),
                                         ptr(support) if n_targets > 0 else None, stream_ptr()), "woft_photo_weights")
