"""The case table and the integer reference of the bit-exact conv-engine tests (helper of test_conv_exact_cpu.py and
test_conv_exact_gpu.py, not collected; no GPU, no library).

The idea: feed the kernels values for which every product and every partial sum, in ANY order, is exactly representable in fp32.
Then fp32, bf16x3, bf16, fp16 and f16mx8 on every kernel must return the integer convolution bit for bit -- no tolerance that a
dropped border tap or a wrong 32-channel chunk could hide in, and no second kernel to share a bug with.

Value modes
  "int"     activations, weights, bias, residual, bias_map: integers in [-amp, amp] (amp 3; 1 where statistics are taken), alpha
            in {0.5, 1, 2}.  Exact in bf16, fp16 and block-scaled e4m3 (1, 2 and 3 keep three mantissa bits): the bf16 lo planes
            and the f16mx8 remainders are exactly zero.
  "wsplit"  (fp32, bf16x3) weights k + s 2^-9, k and s in {-1, 0, 1}: bf16(w) and bf16(w - hi) recover w exactly under round to
            nearest and under truncation; the activation lo plane is zero, so the lo * lo term bf16x3 drops is zero.  Sees a
            misplaced wgt_lo / fragment plane 1.
  "asplit"  (fp32, bf16x3) the mirror: activations k + s 2^-9 with |k| <= amp, weights integers in [-1, 1].  Sees the activation
            split of each loader.
  "wrem"    (f16mx8) weights k + s 2^-12, k and s in {-1, 0, 1}: fp16(w) = k and the remainder s 2^-12 is one bit, exact in
            block-scaled e4m3; the activations are integers (fp16 remainder zero, exact in e4m3).  Of the three products
            fp16(a) fp16(w) + mx8(a - fp16(a)) mx8(w) + mx8(a) mx8(w - fp16(w)) the first gives a k, the second is zero and the
            third gives a s 2^-12: the result is a w exactly, and it depends on the fp8 fragments of the weight remainders, their
            pair-of-taps order and their scales -- which "int" mode, with all remainders zero, cannot see.
  "arem"    (f16mx8) the mirror: activations k + s 2^-12, weights integers in [-1, 1].  Sees the loader's fp8 planes and scale
            bytes and the fp8 fragments of the weights themselves.
Every value is a multiple of a power of two u (its "ULP": 1, 2^-9, 2^-12, halved by alpha = 0.5 or an in_norm rstd of 0.5) and the sum
of the absolute values of everything an output accumulates, over u, stays below 2^24: Ref.bound (test_conv_exact_cpu.py asserts
it, and the GPU test asserts it again before it compares).  Where statistics are taken, tile pixels x max y^2 / u^2 < 2^24 as well
(Ref.stat_bound; statistics are compared in "int" mode only -- in the split modes y^2 is a multiple of 2^-18 and cannot be held).

The reference is integer arithmetic: activations and weights x 2^12 as int64, one matrix product of integers per tap (totals far below 2^53), bias / bias_map
x 2^24, alpha x 2, the epilogue on integers, and one exact division by 2^25 into float64.
"""
import zlib
from functools import lru_cache
from typing import NamedTuple

import torch

from woft_amd import conv_select
from woft_amd.conv_select import PAIR_ANY, PAIR_SAME_TAPS, PAIR_SAME_TILES, Kernel

SENTINEL = -777.25          # pre-fill of every output buffer: what a launch must leave outside its columns / rectangle / rows
TAIL_ROWS = 3               # rows of the output buffer behind the last pixel
SA, SW = 1 << 12, 1 << 12   # integer scales of the activations and the weights
SY = SA * SW * 2            # ... of an output (the 2: alpha = 0.5)
ALL, HALF = ("fp32", "bf16x3", "bf16", "fp16"), ("bf16x3", "bf16", "fp16")
REGB_PREC = HALF + ("f16mx8",)
SPLIT_PRECISIONS = ("fp32", "bf16x3")
MODES = ("int", "wsplit", "asplit")              # of fp32 and bf16x3; the other precisions: "int" alone
MX_MODES = ("int", "wrem", "arem")               # of f16mx8
G, H1, H2 = (2, 5, 7), (2, 9, 17), (1, 8, 16)   # M = 70: a ragged tile across the image boundary; one-pixel tails; exactly one tile
RECT = (3, 5, 5, 11)        # on 9 x 17: aligned to no tile
EPI = {"linear": 0, "relu": 1, "res": 4}        # WOFT_EPI_LINEAR, _RELU, _RELU_RES_RELU (include/woft_hip.h; the GPU test asserts them)


class Case(NamedTuple):
    name: str
    kernel: Kernel
    tile_n: int
    nhw: tuple                      # (n, h, w) of the input
    taps: tuple                     # (kh, kw)
    cin: tuple                      # channels per source: (c,) or (c_split, c of the second source)
    cout: int
    precisions: tuple
    tile_m: int = 64                # GATHER: the forced tile; elsewhere ignored by the kernel
    force: bool = True              # halo= / tiles= overrides (False: the selection's own choice must be `kernel`)
    stride: int = 1
    flat_cs: int = 0
    epi: str = "linear"             # linear | relu | res (WOFT_EPI_RELU_RES_RELU with an integer residual)
    alpha: float = 1.0
    co_off: int = 0                 # > 0: the output buffer is 2 * co_off channels wider than cout
    x2_off: int = 0                 # two sources: first channel of the second tensor that is read
    bias_map: bool = False
    stats: bool = False
    in_norm: int = 0
    rect: tuple = None
    amp: int = 3
    refused: str = ""               # non-empty: woft_conv2d must refuse the launch with WOFT_EINVAL; the reason


def _c(name, kernel, tile_n, nhw, taps, cin, cout, precisions, **kw):
    return Case(name, kernel, tile_n, nhw, taps, cin if isinstance(cin, tuple) else (cin,), cout, precisions, **kw)


def _family(prefix, kernel, precisions, plumbing, rect):
    """The rows shared by the 8 x 16 / 4 x 16 pixel-tile kernels (LDS-halo and register-streamed): the halo shapes, every tap
    form, every channel form; plumbing: statistics and in_norm rows; rect: output-rectangle rows."""
    rows = [
        _c(prefix + "_3x3_c32_o64", kernel, 64, H1, (3, 3), 32, 64, precisions),
        _c(prefix + "_1x5_c96_o126_off", kernel, 128, H1, (1, 5), 96, 126, precisions, epi="relu", co_off=8),
        _c(prefix + "_5x1_two_o192_bmap", kernel, 64, H2, (5, 1), (64, 32), 192, precisions, x2_off=8, alpha=2.0, bias_map=True),
        _c(prefix + "_3x3_c32_o128_res", kernel, 128, H2, (3, 3), 32, 128, precisions, epi="res"),
        _c(prefix + "_1x5_two_o64_half", kernel, 64, H1, (1, 5), (64, 32), 64, precisions, x2_off=4, alpha=0.5, epi="relu"),
        _c(prefix + "_5x1_c96_o128", kernel, 128, H1, (5, 1), 96, 128, precisions),
        _c(prefix + "_3x3_c96_o192", kernel, 64, H1, (3, 3), 96, 192, precisions, epi="relu"),
    ]
    if plumbing:
        rows += [
            _c(prefix + "_3x3_stats", kernel, 64, H1, (3, 3), 32, 64, precisions, stats=True, amp=1),
            _c(prefix + "_1x5_stats_o128", kernel, 128, H2, (1, 5), 32, 128, precisions, stats=True, amp=1, alpha=2.0),
            _c(prefix + "_3x3_norm1", kernel, 64, H1, (3, 3), 96, 64, precisions, in_norm=1),
            _c(prefix + "_3x3_norm2_stats", kernel, 64, H1, (3, 3), 32, 64, precisions, in_norm=2, stats=True, amp=1),
            _c(prefix + "_3x3_norm2_o128", kernel, 128, H2, (3, 3), 96, 128, precisions, in_norm=2, epi="relu"),
        ]
    if rect:
        rows += [
            _c(prefix + "_3x3_rect", kernel, 64, H1, (3, 3), 96, 64, precisions, rect=RECT, epi="relu", alpha=0.5),
            _c(prefix + "_5x1_rect_corner", kernel, 128, H1, (5, 1), 32, 128, precisions, rect=(8, 16, 1, 1)),
            _c(prefix + "_1x5_rect_two", kernel, 64, H1, (1, 5), (64, 32), 64, precisions, rect=(0, 0, 9, 3), x2_off=8),
        ]
    return rows


def _regb12(name, nhw, taps, cin, cout, **kw):
    return _c("regb12_" + name, Kernel.REGB_4X16X128, 128, nhw, taps, cin, cout, REGB_PREC, **kw)


def _gemm(name, nhw, taps, cin, cout, **kw):
    return _c("gemm_" + name, Kernel.GEMM_1X1, 128 if kw.get("flat_cs") else 256, nhw, taps, cin, cout, HALF, force=False, **kw)


def _stem(name, nhw, cout, **kw):
    return _c("stem_" + name, Kernel.STEM, 64, nhw, (7, 7), 3, cout, HALF, **{**dict(force=False, stride=2, flat_cs=4), **kw})


def _win(name, precisions=("bf16x3", "bf16"), **kw):
    return _c("win_" + name, Kernel.WINDOW_9X9, 128, (5, 9, 9), (3, 3), 128, 128, precisions, **kw)


CASES = [
    # ---- GATHER: every tile form, M = 70, every tap form, strides, flat packings ------------------------------------------------
    _c("gather_3x3_c32_o64", Kernel.GATHER, 64, G, (3, 3), 32, 64, ALL),
    _c("gather_1x5_c96_o64_m128", Kernel.GATHER, 64, G, (1, 5), 96, 64, ALL, tile_m=128, epi="relu", alpha=2.0),
    _c("gather_5x1_two_o126_off", Kernel.GATHER, 128, G, (5, 1), (64, 32), 126, ALL, x2_off=8, co_off=8, epi="relu"),
    _c("gather_1x1_c96_o192_bmap", Kernel.GATHER, 128, G, (1, 1), 96, 192, ALL, tile_m=128, alpha=0.5, bias_map=True),
    _c("gather_3x3_s2_res", Kernel.GATHER, 64, G, (3, 3), 32, 64, ALL, stride=2, epi="res"),
    _c("gather_1x1_s2_c96", Kernel.GATHER, 64, G, (1, 1), 96, 64, ALL, stride=2),
    _c("gather_flat7_cs4", Kernel.GATHER, 64, G, (7, 7), 3, 64, ALL, flat_cs=4, epi="relu"),
    _c("gather_flat7_cs4_s2", Kernel.GATHER, 64, (2, 13, 9), (7, 7), 3, 64, ALL, flat_cs=4, stride=2),
    _c("gather_flat3_cs8_o128", Kernel.GATHER, 128, G, (3, 3), 5, 128, ALL, flat_cs=8, tile_m=128),
    _c("gather_3x3_o192_trim", Kernel.GATHER, 64, G, (3, 3), 32, 192, ALL),
    _c("gather_3x3_stats", Kernel.GATHER, 64, G, (3, 3), 32, 64, ALL, stats=True, amp=1),
    _c("gather_3x3_stats_m128_o128", Kernel.GATHER, 128, H1, (3, 3), 32, 128, ALL, tile_m=128, stats=True, amp=1),
    _c("gather_1x1_two_o64", Kernel.GATHER, 64, H1, (1, 1), (64, 32), 64, ALL, x2_off=4),
    # ---- HALO_8X16 / HALO_4X16 -----------------------------------------------------------------------------------------------
    *_family("halo8", Kernel.HALO_8X16, HALF, True, False),
    *_family("halo4", Kernel.HALO_4X16, HALF, True, False),
    # ---- WINDOW_9X9: five 9 x 9 windows ----------------------------------------------------------------------------------------
    _win("linear"),
    _win("relu_half_off", epi="relu", alpha=0.5, co_off=8),
    _win("stats", stats=True, amp=1),
    _win("bmap", bias_map=True, alpha=2.0),
    _win("res", epi="res"),
    # ---- STEM: 13 x 9 -> 7 x 5 (less than a tile), 18 x 34 -> 9 x 17 (crosses the 8 x 16 tiles) ---------------------------------
    _stem("13x9_stats", (1, 13, 9), 64, stats=True, amp=1),
    _stem("18x34_relu_off", (2, 18, 34), 64, epi="relu", alpha=2.0, co_off=8),
    _stem("18x34_stats", (2, 18, 34), 64, stats=True, amp=1),
    _stem("13x9_res", (2, 13, 9), 64, epi="res"),
    _stem("18x34_o126", (1, 18, 34), 126, alpha=0.5, co_off=8),
    # ---- REGB_8X16 -------------------------------------------------------------------------------------------------------------
    *_family("regb8", Kernel.REGB_8X16, REGB_PREC, False, True),
    # ---- REGB_4X16X128 ---------------------------------------------------------------------------------------------------------
    _regb12("1x5_c96_o128", H1, (1, 5), 96, 128, epi="relu"),
    _regb12("5x1_two_o126_off", H2, (5, 1), (64, 32), 126, x2_off=8, co_off=8),
    _regb12("3x3_c32_o192_bmap", H1, (3, 3), 32, 192, bias_map=True, alpha=2.0),
    _regb12("5x1_rect", H1, (5, 1), 32, 128, rect=RECT, alpha=0.5),
    _regb12("3x3_res", H2, (3, 3), 96, 128, epi="res"),
    _regb12("1x5_c32_o128", H2, (1, 5), 32, 128),
    # ---- GEMM_1X1: the selection's own choice (256 columns; flat: 128) ------------------------------------------------------------
    _gemm("1x1_c96_o256_m70", G, (1, 1), 96, 256, epi="relu"),
    _gemm("1x1_two_o254_off", H1, (1, 1), (64, 32), 254, x2_off=8, co_off=8, alpha=0.5),
    _gemm("1x1_c96_o192_bmap", G, (1, 1), 96, 192, bias_map=True, alpha=2.0),
    _gemm("1x1_c32_o256_res", H1, (1, 1), 32, 256, epi="res"),
    _gemm("1x1_c96_rect", H1, (1, 1), 96, 256, rect=RECT, epi="relu"),
    _gemm("flat7_c2", H1, (7, 7), 2, 128, flat_cs=4),
    _gemm("flat7_c2_m70", G, (7, 7), 2, 128, flat_cs=4, epi="relu", alpha=2.0),
    _gemm("flat7_rect", H1, (7, 7), 2, 128, flat_cs=4, rect=RECT),
    _gemm("flat3_cs8_m70", G, (3, 3), 7, 128, flat_cs=8, epi="relu"),
    # ---- refusals: woft_conv2d answers WOFT_EINVAL and writes nothing -------------------------------------------------------------
    _win("fp16_refused", precisions=("fp16",), refused="the 9 x 9 window kernel keeps the split-bf16 arithmetic: no fp16 instance"),
    _c("halo8_rect_refused", Kernel.HALO_8X16, 64, H1, (3, 3), 32, 64, HALF, rect=RECT, refused="no output rectangle on an LDS-halo kernel"),
    _c("gather_rect_refused", Kernel.GATHER, 64, H1, (3, 3), 32, 64, ALL, rect=RECT, refused="no output rectangle on the gather kernel"),
    _c("regb8_stats_refused", Kernel.REGB_8X16, 64, H1, (3, 3), 32, 64, HALF, stats=True, amp=1, refused="no statistics on the register-streamed kernel"),
    _c("halo8_fp32_refused", Kernel.HALO_8X16, 64, H1, (3, 3), 32, 64, ("fp32",), refused="the LDS-halo kernels have no fp32 instance"),
    _stem("bmap_refused", (1, 13, 9), 64, bias_map=True, force=True, refused="no per-pixel bias on the stem kernel"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# woft_conv2d_pair: (the kernel's pair rule, first layer, second layer) -- one launch, each layer against its own reference
PAIRS = [
    (PAIR_SAME_TILES, "gather_3x3_c32_o64", "gather_1x1_s2_c96"),
    (PAIR_SAME_TILES, "gather_flat7_cs4", "gather_3x3_o192_trim"),
    (PAIR_SAME_TAPS, "regb8_3x3_c32_o64", "regb8_3x3_rect"),
    (PAIR_SAME_TAPS, "regb12_1x5_c96_o128", "regb12_1x5_c32_o128"),
    (PAIR_ANY, "gemm_1x1_c96_o256_m70", "gemm_flat7_c2"),
    (PAIR_ANY, "gemm_flat7_rect", "gemm_1x1_two_o254_off"),
]


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def _round_up(x, m):
    return (x + m - 1) // m * m


def padding(case):
    return case.taps[0] // 2, case.taps[1] // 2


def out_hw(case):
    (kh, kw), (py, px), (_, h, w) = case.taps, padding(case), case.nhw
    return (h + 2 * py - kh) // case.stride + 1, (w + 2 * px - kw) // case.stride + 1


def cout_pad(case):
    """ops.pack_conv's rule."""
    return _round_up(case.cout, 64) if case.cout <= 64 else _round_up(case.cout, 128)


def cin_pad(case):
    return 32 if case.flat_cs else _round_up(sum(case.cin), 32)


def ldo(case):
    return _round_up(case.cout + 2 * case.co_off, 4)


def overrides(case):
    """-> (tiles, halo) of conv_select.select / ops.conv_params."""
    if not case.force:
        return None, None
    return (case.tile_m, case.tile_n), int(case.kernel)


def layer(case):
    """The conv_select.Layer that ops.conv_params derives from the case's operands."""
    (n, h, w), (ho, wo), (py, px) = case.nhw, out_hw(case), padding(case)
    taps = (case.taps[0], 1) if case.flat_cs else case.taps
    cs0 = case.flat_cs or _round_up(case.cin[0], 32)
    return conv_select.Layer(n, h, w, ho, wo, taps[0], taps[1], case.stride, py, px, cin_pad(case), case.cout, cout_pad(case),
                             int(bool(case.flat_cs)), cs0, len(case.cin) == 2, case.stats, case.in_norm, case.bias_map, False,
                             EPI[case.epi])


def selection(case, precision):
    tiles, halo = overrides(case)
    return conv_select.select(layer(case), conv_select.PRECISION[precision], conv_select.Switches(mx_layers="all"), tiles, halo)


def modes(case, precision):
    return MX_MODES if precision == "f16mx8" else MODES if precision in SPLIT_PRECISIONS else MODES[:1]


def all_modes(case):
    """The value modes of a row: those of its precisions, "int" first."""
    return tuple(dict.fromkeys(m for p in case.precisions for m in modes(case, p)))


def tile_pixels(case):
    """Pixels of a workgroup tile: no partial statistics row totals more."""
    tile = conv_select.KERNELS[case.kernel].tile
    return case.tile_m if tile is None else tile[0] * tile[1]


# ---- values ---------------------------------------------------------------------------------------------------------------------
def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64)


class Inputs(NamedTuple):
    """Integer operands: x at scale SA, w at scale SW, bias / bias_map / res at scale 1 (plain integers); mean an integer other
    than 0 and rstd2 = 2 * rstd in {1, 2, 4} per input channel (in_norm rows)."""
    x: torch.Tensor                 # (n, cin, h, w)
    w: torch.Tensor                 # (cout, cin, kh, kw)
    bias: torch.Tensor              # (cout,)
    bias_map: torch.Tensor          # (n, cout, ho, wo) or None
    res: torch.Tensor               # (n, cout, ho, wo) or None
    mean: torch.Tensor              # (cin,) or None
    rstd2: torch.Tensor             # (cin,) or None


@lru_cache(maxsize=None)
def inputs(case, mode):
    """The case's operands in a value mode: deterministic, shared between the tests, never modified."""
    gen = torch.Generator().manual_seed(zlib.crc32(f"{case.name}/{mode}".encode()))
    (n, h, w), (ho, wo), cin, a = case.nhw, out_hw(case), sum(case.cin), case.amp
    x = _ints(gen, (n, cin, h, w), -a, a) * SA
    wt = _ints(gen, (case.cout, cin) + case.taps, -a, a) * SW
    fine = {"wsplit": SW >> 9, "asplit": SA >> 9, "wrem": SW >> 12, "arem": SA >> 12}.get(mode)
    if mode in ("wsplit", "wrem"):
        wt = _ints(gen, wt.shape, -1, 1) * SW + _ints(gen, wt.shape, -1, 1) * fine
    elif mode in ("asplit", "arem"):
        x = x + _ints(gen, x.shape, -1, 1) * fine
        wt = _ints(gen, wt.shape, -1, 1) * SW
    bias = _ints(gen, (case.cout,), -a, a)
    shape = (n, case.cout, ho, wo)
    bias_map = _ints(gen, shape, -a, a) if case.bias_map else None
    res = _ints(gen, shape, -3, 3) if case.epi == "res" else None
    mean = rstd2 = None
    if case.in_norm:
        mean = _ints(gen, (cin,), 1, 2) * (2 * _ints(gen, (cin,), 0, 1) - 1)
        rstd2 = 1 << _ints(gen, (cin,), 0, 2)
    return Inputs(x, wt, bias, bias_map, res, mean, rstd2)


def as_float(t, scale):
    """An integer operand as the float64 value it stands for (exact)."""
    return t.double() / scale


def _granule(t):
    """The largest power of two that divides every entry of an integer tensor (2^40 for all zeros)."""
    g = 1 << 40
    while bool((t % g != 0).any()):
        g >>= 1
    return g


# ---- the reference --------------------------------------------------------------------------------------------------------------
def conv_int(x, w, stride, pad_y, pad_x, ho, wo):
    """sum over taps and channels of x[n, c, oy * stride - pad_y + ky, ox * stride - pad_x + kx] * w[o, c, ky, kx] as integers, zeros
    outside the image."""
    n, c, h, wd = x.shape
    co, _, kh, kw = w.shape
    out = torch.zeros(n, co, ho, wo, dtype=torch.int64)
    oy, ox = torch.arange(ho) * stride - pad_y, torch.arange(wo) * stride - pad_x
    for ky in range(kh):
        iy = oy + ky
        vy = (iy >= 0) & (iy < h)
        for kx in range(kw):
            ix = ox + kx
            vx = (ix >= 0) & (ix < wd)
            patch = x[:, :, iy.clamp(0, h - 1)][:, :, :, ix.clamp(0, wd - 1)] * (vy[:, None] & vx[None, :])
            # (the product of a tap as a float64 matrix product of integers: every partial sum is an integer below 2^53, hence exact)
            out += torch.einsum("nchw,oc->nohw", patch.double(), w[:, :, ky, kx].double()).long()
    return out


def normalised(case, inp):
    """The conv's input at scale SA: in_norm rows (x - mean) * rstd (2: + ReLU); the zero padding comes after it (conv_int)."""
    if not case.in_norm:
        return inp.x
    xn = (inp.x - inp.mean.view(1, -1, 1, 1) * SA) * inp.rstd2.view(1, -1, 1, 1)
    assert bool((xn % 2 == 0).all())
    xn = xn // 2
    return xn.clamp(min=0) if case.in_norm == 2 else xn


class Ref(NamedTuple):
    out: torch.Tensor               # (n, cout, ho, wo) float64: the launch's output values
    buffer: torch.Tensor            # (n * ho * wo + TAIL_ROWS, ldo) float64: the whole output buffer, SENTINEL where nothing is written
    stat_sum: torch.Tensor          # (cout,) float64: sum over all pixels of y = alpha * acc + bias (before the activation)
    stat_sq: torch.Tensor           # (cout,) float64: sum of y^2
    x_norm: torch.Tensor            # (n, cin, h, w) float64: the conv's input after in_norm
    bound: float                    # largest sum of |terms| of an output over the values' ULP; must stay below 2^24
    stat_bound: float               # pixels of a partial statistics row * max y^2 / ULP^2; must stay below 2^24


def reference(case, mode, inp=None, pad_shift=(0, 0)):
    """The expected result of a case in a value mode.  inp: other operands than inputs(case, mode); pad_shift: the padding moved
    by that many pixels (the sensitivity checks of test_conv_exact_cpu.py)."""
    inp = inp or inputs(case, mode)
    (ho, wo), (py, px), n = out_hw(case), padding(case), case.nhw[0]
    xn = normalised(case, inp)
    acc = conv_int(xn, inp.w, case.stride, py + pad_shift[0], px + pad_shift[1], ho, wo)         # scale SA * SW
    b = (inp.bias_map if case.bias_map else inp.bias.view(1, -1, 1, 1)) * (SA * SW)              # (a per-pixel bias replaces the bias)
    a2 = int(round(2 * case.alpha))
    assert a2 in (1, 2, 4)
    y = acc * a2 + b * 2                                                                         # scale SY
    out = y
    if case.epi in ("relu", "res"):
        out = out.clamp(min=0)
    if case.epi == "res":
        out = (out + inp.res * SY).clamp(min=0)
    # exactness: everything an accumulator or the epilogue holds is a multiple of `ulp` (in units of 1 / SY) ...
    absacc = conv_int(xn.abs(), inp.w.abs(), case.stride, py, px, ho, wo) * a2 + b.abs() * 2
    if case.epi == "res":
        absacc = absacc + inp.res.abs() * SY
    #     from the operands' own granularity, not from the totals: a partial sum is as fine as its terms
    u_acc = _granule(xn) * _granule(inp.w) * 2                                                   # products, at scale SY
    ulp = min(u_acc, u_acc * a2 // 2, _granule(b) * 2, SY)
    bound = float(absacc.max()) / ulp * max(1.0, 1.0 / case.alpha)                               # (the accumulator itself is y / alpha)
    stat_bound = float(tile_pixels(case)) * (float(y.abs().max()) / ulp) ** 2 if case.stats else 0.0
    outf, yf = out.double() / SY, y.double() / SY
    buf = torch.full((n * ho * wo + TAIL_ROWS, ldo(case)), SENTINEL, dtype=torch.float64)
    rows = outf.permute(0, 2, 3, 1).reshape(n * ho * wo, case.cout)
    inside = torch.ones(ho, wo, dtype=torch.bool)
    if case.rect:
        y0, x0, rh, rw = case.rect
        inside[:] = False
        inside[y0:y0 + rh, x0:x0 + rw] = True
    m = inside.reshape(1, -1).expand(n, -1).reshape(-1)
    view = buf[:n * ho * wo, case.co_off:case.co_off + case.cout]
    view[m] = rows[m]
    return Ref(outf, buf, yf.sum(dim=(0, 2, 3)), (yf * yf).sum(dim=(0, 2, 3)), as_float(xn, SA), bound, stat_bound)
