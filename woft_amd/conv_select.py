"""Which kernel instance a convolution layer runs on: the kernels by name, one table of what each takes, one rule per kernel.

Pure: integers and flags in, an immutable Selection out -- no tensors, no ctypes, no library (tests/test_conv_select_cpu.py pins
every outcome without a GPU).  ops.conv_params derives a Layer from its operands, calls select() and fills a woft_conv_params
from the result; the engine asks select() directly where it only needs the answer.

The kernels' values are the numbers of woft_conv_params.halo (include/woft_hip.h): the field long ago stopped meaning a halo size.
"""
import math
from enum import IntEnum
from typing import NamedTuple

PRECISION = {"fp32": 0, "bf16x3": 1, "bf16": 2, "fp16": 3, "f16mx8": 4}
FP32, BF16X3, BF16, FP16, F16MX8 = range(5)
EPI_FLOWHEAD = 9                    # WOFT_EPI_FLOWHEAD (ops asserts that it is _lib's)


class Kernel(IntEnum):
    GATHER = 0          # per-tap gather kernel (conv.hip): every shape and precision, tile_m x tile_n tiles of the linear pixel order
    HALO_8X16 = 1       # LDS-halo kernel on 8 x 16 pixel tiles (conv.hip)
    WINDOW_9X9 = 2      # LDS-halo kernel on one whole 9 x 9 window per workgroup, 128 columns (conv.hip; the weight head)
    HALO_4X16 = 4       # LDS-halo kernel on 4 x 16 pixel tiles
    STEM = 7            # the encoders' 7x7 / stride-2 first layer on the NHWC4 image (conv_stem.hip)
    REGB_8X16 = 8       # weights streamed global -> registers, 8 x 16 pixel tiles (conv_regb.hip)
    REGB_4X16X128 = 12  # ... 4 x 16 pixels x 128 columns: the four waves are four column bands
    GEMM_1X1 = 16       # streamed 1x1 / flat GEMM, 64-pixel runs x 256 or 128 columns (conv_1x1.hip)


RUNS_64 = "64-pixel runs"                                    # KernelInfo.tile of the GEMM kernel
PAIR_SAME_TILES, PAIR_SAME_TAPS, PAIR_ANY = "same tile_m and tile_n", "same tile_n and taps, multi-tap", "any two layers"
SPLIT, FRAG = "wgt_hi / wgt_lo", "wgt_frag (+ wgt_mx in f16mx8)"


class KernelInfo(NamedTuple):
    tile: object        # (TY, TX) pixels of a workgroup; RUNS_64; None: tile_m pixels of the linear order
    roi: bool           # takes an output rectangle (woft_conv_params.roi_*)
    stats: bool         # writes InstanceNorm partial statistics (stat_sum / stat_sq)
    in_norm: bool       # normalises a raw input on load (in_norm / in_mean / in_rstd; instantiated for 3x3 taps)
    pair: str           # how woft_conv2d_pair takes two layers of it (None: not at all)
    weights: str        # the weight form it reads


KERNELS = {
    Kernel.GATHER:        KernelInfo(None,    False, True,  False, PAIR_SAME_TILES, SPLIT),
    Kernel.HALO_8X16:     KernelInfo((8, 16), False, True,  True,  None,            SPLIT),
    Kernel.WINDOW_9X9:    KernelInfo((9, 9),  False, True,  False, None,            SPLIT),
    Kernel.HALO_4X16:     KernelInfo((4, 16), False, True,  True,  None,            SPLIT),
    Kernel.STEM:          KernelInfo((8, 16), False, True,  False, None,            SPLIT),
    Kernel.REGB_8X16:     KernelInfo((8, 16), True,  False, False, PAIR_SAME_TAPS,  FRAG),
    Kernel.REGB_4X16X128: KernelInfo((4, 16), True,  False, False, PAIR_SAME_TAPS,  FRAG),
    Kernel.GEMM_1X1:      KernelInfo(RUNS_64, True,  False, False, PAIR_ANY,        FRAG),
}
REGB = (Kernel.REGB_8X16, Kernel.REGB_4X16X128)
HALO_TAPS = ((3, 3), (1, 5), (5, 1))                         # the LDS-halo and register-streamed kernels' instances


class Layer(NamedTuple):
    """What the selection reads of a layer and its operands."""
    n: int
    h: int
    w: int
    ho: int
    wo: int
    taps_y: int
    taps_x: int
    stride: int
    pad_y: int
    pad_x: int
    cin_pad: int
    cout: int           # valid output channels of this launch (conv_params' cout override)
    cout_pad: int       # rows of the packed weight matrix
    flat: int
    cs0: int            # channel stride of the input
    x2: bool            # a second source
    stats: bool         # InstanceNorm statistics asked for
    in_norm: int        # 1 / 2: the input is a raw conv output to normalise (+ ReLU) on load
    bias_map: bool
    wh0: bool           # the weight head's first conv evaluated inside this launch
    epi: int


class Switches(NamedTuple):
    """Developer switches (ops' module attributes of these names in upper case, WOFT_MX_ZR), defaults as ops reads them."""
    use_halo: bool = True
    use_regb: bool = True
    regb_ty4: bool = True
    use_stem: bool = True
    use_1x1: bool = True
    wh_halo: int = 2
    halo_min_blocks: int = 400
    tile_min_blocks: int = 400
    mx_layers: str = "auto"
    mx_zr: str = "12"


class Selection(NamedTuple):
    kernel: Kernel
    tile_m: int
    tile_n: int
    cout_pad: int       # columns launched (trimmed from the packed cout_pad where whole column tiles are padding)
    precision: int      # effective: f16mx8 is demoted to bf16x3 where it has no instance or measured slower
    in_norm: int        # effective: 0 where the kernel cannot normalise on load (the caller applies woft_inorm_apply)
    m_tiles: int        # pixel tiles of the launch (the statistics have two rows per tile)


def _round_up(x, m):
    return (x + m - 1) // m * m


def _cdiv(a, b):
    return -(-a // b)


def pick_tiles(m, cout_pad, tile_min_blocks=400):
    """Block tile: 128-wide in N when the padded cout allows; 128 rows in M when that still yields
    at least tile_min_blocks workgroups (256 CUs), else 64."""
    tn = 128 if cout_pad % 128 == 0 else 64
    blocks128 = math.ceil(m / 128) * (cout_pad // tn)
    tm = 128 if blocks128 >= tile_min_blocks else 64
    return tm, tn


def launched_cout_pad(l, kernel, tile_n):
    """Columns actually launched: with statistics the rows keep the padded width; else whole column tiles of padding are
    dropped (convc2, cout 192 in 256 rows: 3 instead of 4 x 64)."""
    if l.stats:
        return l.cout_pad
    if kernel in REGB:
        return _round_up(l.cout, tile_n)
    return _round_up(l.cout, 64) if tile_n == 64 else l.cout_pad


def m_tiles(l, kernel, tile_m):
    tile = KERNELS[kernel].tile
    if tile in (None, RUNS_64):
        return math.ceil(l.n * l.ho * l.wo / tile_m)
    return l.n * math.ceil(l.ho / tile[0]) * math.ceil(l.wo / tile[1])


def roi_tiles(kernel, rect, hf, wf):
    """Workgroups per column tile of a launch of an output-rectangle kernel on rect = (y0, x0, h, w) (None: the whole hf x wf map)."""
    tile = KERNELS[kernel].tile
    y0, x0, h, w = rect or (0, 0, hf, wf)
    if tile == RUNS_64:                                      # along the rectangle's rows / of the linear pixel order
        return h * _cdiv(w, 64) if rect else _cdiv(hf * wf, 64)
    return _cdiv(h, tile[0]) * _cdiv(w, tile[1])


def pair_ok(a, b):
    """True when woft_conv2d_pair takes the two layers (filled woft_conv_params) in one launch: the same kernel instance."""
    if a.precision == FP32 or a.precision != b.precision or a.halo != b.halo or a.stat_sum or b.stat_sum:
        return False
    pair = KERNELS[Kernel(a.halo)].pair
    if pair is None or pair == PAIR_ANY:                     # (PAIR_ANY: a kernel whose workgroups pick their layer's tile form)
        return pair is not None
    if a.tile_n != b.tile_n or a.in_norm or b.in_norm:
        return False
    if pair == PAIR_SAME_TILES:                              # (the pixel-tile kernels ignore tile_m)
        return a.tile_m == b.tile_m
    return (a.taps_y, a.taps_x) == (b.taps_y, b.taps_x) and a.taps_y * a.taps_x > 1


# ---- eligibility: one rule per kernel ------------------------------------------------------------------------------
def _taps(l):
    return (l.taps_y, l.taps_x)


def _same_size(l):
    return (l.ho, l.wo) == (l.h, l.w)


def _halo_shape(l, precision):
    """Shapes the LDS-halo kernels (1, 2, 4) and the register-streamed ones (8, 12) are instantiated for: the split-bf16
    precisions on stride-1 multi-tap convs (see conv.hip)."""
    return precision != FP32 and not l.flat and l.stride == 1 and _same_size(l) and _taps(l) in HALO_TAPS


def _plumbing_ok(l, kernel):
    """The layer asks for no InstanceNorm plumbing that the kernel does not take."""
    return (KERNELS[kernel].stats or not l.stats) and (KERNELS[kernel].in_norm or not l.in_norm)


def _gather_tiles(l, precision, sw):
    m = l.n * l.ho * l.wo
    tm, tn = pick_tiles(m, l.cout_pad, sw.tile_min_blocks)
    if precision == FP32 and tm == 128 and math.ceil(m / 128) * (l.cout_pad // tn) < 2048:
        tm = 64                         # fp32 kernel: 64-row tiles up to ~2000 workgroups (3-15 % per layer, gather_sweep.py fp32)
    if precision != FP32 and (l.flat or l.taps_y * l.taps_x == 1):
        tm, tn = 64, 64                 # short-K gather layers (1x1, flat 7x7): 64 x 64 tiles measured 5-35 % faster
                                        # than 128-wide ones at every resolution of a 1080p frame (tools/gather_sweep.py)
    if tn == 128 and not l.stats and _round_up(l.cout, 64) < l.cout_pad:
        tn = 64                         # the last 64 columns of the 128-padded weight matrix are padding (cout 192, 576)
    return tm, tn


def _lds_halo(l, precision, sw, auto, tn):
    """-> (HALO_8X16 | HALO_4X16 | WINDOW_9X9, else GATHER; tile_n): the LDS-halo kernels; auto: the caller gave no tiles."""
    if not (sw.use_halo and _halo_shape(l, precision)):
        return Kernel.GATHER, tn
    if (l.h, l.w) == (9, 9) and tn == 128:
        return Kernel(sw.wh_halo if l.n >= 4 * 256 else Kernel.WINDOW_9X9), tn
    if not (l.h >= 8 and l.w >= 16):
        return Kernel.GATHER, tn
    # Tile choice, measured on MI355X with tools/tile_sweep.py (1080p layer shapes).  Many independent
    # workgroups beat larger tiles (16x16 / multi-patch workgroups run at 1 block per CU and lose to
    # 8x16 by 1.5-3x): take the 8x16 pixel tile only while it still yields ~2 workgroups per CU, else 4x16.
    b816 = l.n * math.ceil(l.ho / 8) * math.ceil(l.wo / 16)
    if auto and precision in (BF16, FP16):
        # plain bf16 (one LDS plane, fewer registers): 64-channel column tiles win throughout --
        # 8x16 x 64 for the 256-wide layers (~1000 workgroups), 4x16 x 64 for the narrower ones
        cols = launched_cout_pad(l, Kernel.HALO_8X16, 64) // 64
        return (Kernel.HALO_8X16 if 4 * b816 * cols >= 7 * sw.halo_min_blocks else Kernel.HALO_4X16), 64   # (>= 700 workgroups)
    # bf16x3: 64-channel column tiles (three workgroups per CU) unless their grid lands just over
    # one round of the 768 resident slots while the 128-wide tiles (two per CU) still fit in one
    # round -- the 256-wide layers at 1/8 of 1080p; 4x16 pixel tiles when 8x16 gives too few workgroups
    if auto and tn == 128:
        w64 = b816 * math.ceil(l.cout / 64)
        wide_ok = l.cout_pad % 128 == 0 and b816 * (l.cout_pad // 128) <= 512
        if not (wide_ok and 768 < w64 < 1536):
            tn = 64
    cols = launched_cout_pad(l, Kernel.HALO_8X16, tn) // tn
    return (Kernel.HALO_8X16 if b816 * cols >= sw.halo_min_blocks else Kernel.HALO_4X16), tn


def _stem(l, precision, sw):
    """The encoders' first layer (7x7, stride 2, 3 -> 64 on the NHWC4 image, flat packing): its own kernel (conv_stem.hip) --
    bit-identical to the gather kernel, 8x16-pixel tiles (the statistics rows follow them)."""
    return (sw.use_stem and precision != FP32 and l.flat and l.cs0 == 4 and not l.x2
            and (l.taps_y, l.taps_x, l.stride, l.pad_y, l.pad_x, l.cin_pad) == (7, 1, 2, 3, 3, 32)
            and l.cout_pad % 64 == 0 and _plumbing_ok(l, Kernel.STEM) and not l.bias_map and not l.wh0
            and (l.ho, l.wo) == ((l.h - 1) // 2 + 1, (l.w - 1) // 2 + 1))


def _regb(l, sw, halo_kernel, tn):
    """Stride-1 multi-tap layers without InstanceNorm plumbing, wherever the 8x16 / 4x16 LDS-halo kernel was chosen: the kernel
    that streams the weights global -> registers (conv_regb.hip) -- bit-identical, 1-8 % faster per layer on the update block's
    shapes (tools/regb_check.py).  -> (kernel, tile_n) or None."""
    if not (sw.use_regb and halo_kernel in (Kernel.HALO_8X16, Kernel.HALO_4X16) and _plumbing_ok(l, Kernel.REGB_8X16)):
        return None
    if halo_kernel == Kernel.HALO_4X16:
        tn = 64
    # the GRU q convs (1x5 / 5x1, 128 columns) on 4x16-pixel x 128-column tiles instead of 8x16 x 64: same workgroup count and
    # per-wave work (64 rows x 32 columns), but the four waves are four column bands -- the weight fragments are fetched once
    # per workgroup instead of by both row halves.  Alone -6...8 % per layer at 1/8 of 1080p; inside a frame +-0 at 1080p
    # and 4K, +1.5 % frames/s at 720p.  (convm the same alone, nothing in a frame: left on 8x16 x 64; a layer that would pad
    # to 128 columns -- convc2, 192 -> 256 -- loses 19 %.)  WOFT_REGB_TY4=0: off
    if sw.regb_ty4 and tn == 64 and l.cout_pad % 128 == 0 and _round_up(l.cout, 64) == l.cout_pad and _taps(l) in ((1, 5), (5, 1)):
        return Kernel.REGB_4X16X128, 128
    return Kernel.REGB_8X16, tn


def _gemm(l, precision, sw):
    """-> tile_n of the streamed GEMM kernel (conv_1x1.hip) or None.  Wide 1x1 / stride-1 layers (convc1: 324 -> 256; the
    encoders' closing 128 -> 256): 64 pixels x all 256 columns per workgroup, activations read and converted once per layer;
    bit-identical to the gather kernel.  (Layers that only fill 128-column tiles gain nothing: mask head conv2 256 -> 576 61.5 vs
    59.9 us, 128 -> 128 13.8 vs 14.0.)  And the flat-packed 7x7 conv on the flow (convf1, update.py:91) on the same kernel (128
    columns per workgroup, K chunks = tap rows), so that it keeps sharing convc1's launch (pair_ok)."""
    if not (sw.use_1x1 and precision != FP32 and _plumbing_ok(l, Kernel.GEMM_1X1) and not l.wh0 and _same_size(l)):
        return None
    if not l.flat and (l.taps_y, l.taps_x, l.stride, l.pad_y, l.pad_x) == (1, 1, 1, 0, 0) \
            and l.cout_pad % 256 == 0 and _round_up(l.cout, 256) == l.cout_pad:
        return 256
    if l.flat and not l.x2 and (l.taps_x, l.stride, l.cin_pad) == (1, 1, 32) and 2 * l.pad_y + 1 == l.taps_y \
            and l.cout_pad % 128 == 0 and _round_up(l.cout, 128) == l.cout_pad:
        return 128
    return None


def _f16mx8(l, sw, auto, kernel, tile_n):
    """Precision f16mx8 asked for -> (precision, kernel, tile_n).  It exists on the register-streamed kernel's multi-tap
    instances: elsewhere bf16x3."""
    if not (kernel in REGB and l.taps_y * l.taps_x > 1 and not l.in_norm):
        return BF16X3, kernel, tile_n
    if sw.mx_layers == "auto":
        # measured per layer at 1080p (profiles/r04_layer_times_f16mx8*.txt against ..._bf16x3.txt): the 3x3 layers are 8-10 % faster in
        # f16mx8 than in bf16x3 (motion encoder, flow head, context encoder); the GRU's 1x5 / 5x1 z|r layers are 4-7 % slower (four row
        # tiles per wave do not fit the 256 registers: half-size workgroups), the q layers equal, and the 128-column instance with a
        # full-width store epilogue (mask head conv: spills) 75 vs 55 us -> those stay bf16x3
        tn_mx = tile_n if tile_n in (64, 128) else (128 if l.cout_pad % 128 == 0 else 64)
        if _taps(l) != (3, 3) or (tn_mx == 128 and l.cout_pad % 128 == 0 and l.epi != EPI_FLOWHEAD):
            return BF16X3, kernel, tile_n
    if kernel == Kernel.REGB_8X16 and auto and tile_n == 128:
        # two row tiles per wave have the registers for the deep fragment pipeline; four (8 x 16 pixels x 128 columns) spill:
        # 1x5 / 5x1 layers take the 4 x 16-pixel x 128-column layout (WOFT_MX_ZR = 12; 64: 64-column tiles; 128: keep)
        # (3x3 layers keep their 128-column choice: that instance spills 40 bytes and still beats 64 columns, 52.7 vs 58.8 us on fh1)
        if _taps(l) in ((1, 5), (5, 1)) and l.cout_pad % 128 == 0 and _round_up(l.cout, 128) == l.cout_pad and sw.mx_zr == "12":
            kernel = Kernel.REGB_4X16X128
        elif _taps(l) != (3, 3) and sw.mx_zr == "64":
            tile_n = 64
    return F16MX8, kernel, tile_n


def select(l, precision, sw=Switches(), tiles=None, halo=None):
    """The kernel instance of layer l (a Layer) in `precision` (a number of PRECISION).  tiles = (tile_m, tile_n) and halo (a
    Kernel or its number) are the caller's overrides: given tiles keep the layer off every kernel with a tiling of its own, a
    given kernel is taken as it is, and a combination that no kernel is instantiated for is the caller's business (the library
    refuses it).  -> Selection."""
    auto = tiles is None
    tm, tn = tiles or _gather_tiles(l, precision, sw)
    if halo is not None:
        kernel = Kernel(halo)
    else:
        kernel, tn = _lds_halo(l, precision, sw, auto, tn)
        if auto:                        # (given tiles keep the layer off the kernels that bring their own)
            regb, gemm_tn = _regb(l, sw, kernel, tn), _gemm(l, precision, sw)
            if regb is not None:
                kernel, tn = regb
            elif kernel == Kernel.GATHER and _stem(l, precision, sw):
                kernel, tn = Kernel.STEM, 64
            elif kernel == Kernel.GATHER and gemm_tn is not None:
                kernel, tm, tn = Kernel.GEMM_1X1, 64, gemm_tn
    if precision == F16MX8:
        precision, kernel, tn = _f16mx8(l, sw, auto, kernel, tn)
    if kernel in REGB:                  # (an override may have brought the layer here)
        assert _halo_shape(l, precision) and (KERNELS[kernel].in_norm or not l.in_norm)
        if kernel == Kernel.REGB_4X16X128:
            assert l.cout_pad % 128 == 0
            tn = 128
        if tn == 128 and l.cout_pad % 128 != 0:
            tn = 64
    if l.wh0:
        assert kernel == Kernel.WINDOW_9X9 and precision != FP32 and l.cin_pad == 128, "fused first layer: 9x9 whole-window kernel only"
    in_norm = l.in_norm if KERNELS[kernel].in_norm and _taps(l) == (3, 3) else 0
    return Selection(kernel, tm, tn, launched_cout_pad(l, kernel, tn), precision, in_norm, m_tiles(l, kernel, tm))
