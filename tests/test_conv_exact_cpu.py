"""The table and the reference of the bit-exact conv tests (tests/conv_exact_cases.py), checked without a GPU: the reference is the
convolution, every case's values stay exact in fp32, every row runs on the kernel instance it names, the table covers the
instances, and no row's inputs are degenerate (a dropped tap, a dropped 32-channel chunk or a shifted padding changes the result)."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))

import conv_exact_cases as cx  # noqa: E402
from woft_amd import conv_select, ops  # noqa: E402
from woft_amd.conv_select import BF16, BF16X3, F16MX8, FP16, FP32, KERNELS, Kernel  # noqa: E402

RUN = [c for c in cx.CASES if not c.refused]
IDS = [c.name for c in RUN]

# what the table must cover: every kernel instance (kernel, tile_n) in every precision it has
COVERAGE = (
    [(Kernel.GATHER, tn, p) for tn in (64, 128) for p in (FP32, BF16X3, BF16, FP16)]
    + [(k, tn, p) for k in (Kernel.HALO_8X16, Kernel.HALO_4X16) for tn in (64, 128) for p in (BF16X3, BF16, FP16)]
    + [(Kernel.WINDOW_9X9, 128, p) for p in (BF16X3, BF16)]
    + [(Kernel.STEM, 64, p) for p in (BF16X3, BF16, FP16)]
    + [(Kernel.REGB_8X16, tn, p) for tn in (64, 128) for p in (BF16X3, BF16, FP16, F16MX8)]
    + [(Kernel.REGB_4X16X128, 128, p) for p in (BF16X3, BF16, FP16, F16MX8)]
    + [(Kernel.GEMM_1X1, tn, p) for tn in (128, 256) for p in (BF16X3, BF16, FP16)]
)
GATHER_TILES = {(64, 64), (128, 64), (64, 128), (128, 128)}


def _float_conv(case, mode):
    """float64 F.conv2d on the values the integers stand for, bias, alpha and epilogue applied in float64."""
    inp = cx.inputs(case, mode)
    x = cx.as_float(inp.x, cx.SA)
    if case.in_norm:
        x = (x - inp.mean.double().view(1, -1, 1, 1)) * (inp.rstd2.double() / 2).view(1, -1, 1, 1)
        x = F.relu(x) if case.in_norm == 2 else x
    y = case.alpha * F.conv2d(x, cx.as_float(inp.w, cx.SW), None, stride=case.stride, padding=cx.padding(case))
    y = y + (inp.bias_map.double() if case.bias_map else inp.bias.double().view(1, -1, 1, 1))
    out = F.relu(y) if case.epi != "linear" else y
    if case.epi == "res":
        out = F.relu(out + inp.res.double())
    return x, y, out


@pytest.mark.parametrize("case", RUN, ids=IDS)
def test_reference_is_the_convolution(case):
    for mode in cx.all_modes(case):
        ref = cx.reference(case, mode)
        x, y, out = _float_conv(case, mode)
        assert tuple(out.shape[2:]) == cx.out_hw(case)
        assert torch.equal(ref.out, out), (mode, float((ref.out - out).abs().max()))
        assert torch.equal(ref.x_norm, x) and torch.equal(ref.stat_sum, y.sum(dim=(0, 2, 3))) and torch.equal(ref.stat_sq, (y * y).sum(dim=(0, 2, 3)))
        # placement: the values at co_off inside the rectangle, the sentinel everywhere else
        n, (ho, wo) = case.nhw[0], cx.out_hw(case)
        buf = ref.buffer
        assert buf.shape == (n * ho * wo + cx.TAIL_ROWS, cx.ldo(case)) and cx.ldo(case) % 4 == 0
        written = buf != cx.SENTINEL
        y0, x0, rh, rw = case.rect or (0, 0, ho, wo)
        assert int(written.sum()) == n * rh * rw * case.cout
        assert not bool(written[:, :case.co_off].any()) and not bool(written[:, case.co_off + case.cout:].any())
        assert not bool(written[n * ho * wo:].any())
        got = buf[:n * ho * wo, case.co_off:case.co_off + case.cout].reshape(n, ho, wo, case.cout).permute(0, 3, 1, 2)
        assert torch.equal(got[:, :, y0:y0 + rh, x0:x0 + rw], out[:, :, y0:y0 + rh, x0:x0 + rw])


@pytest.mark.parametrize("case", RUN, ids=IDS)
def test_values_stay_exact_in_fp32(case):
    """The preconditions of bit-exactness: conditions on the inputs, not tolerances."""
    assert case.alpha in (0.5, 1.0, 2.0) and case.amp in (1, 3)
    for mode in cx.all_modes(case):
        inp, ref = cx.inputs(case, mode), cx.reference(case, mode)
        assert ref.bound < 2 ** 24, (mode, ref.bound)
        if mode == "int":
            assert ref.stat_bound < 2 ** 24, ref.stat_bound
            assert bool((inp.x % cx.SA == 0).all()) and bool((inp.w % cx.SW == 0).all())
            assert int(inp.x.abs().max()) == case.amp * cx.SA and int(inp.w.abs().max()) == case.amp * cx.SW
        # every operand survives the formats it is split into: hi + lo is the value (the bf16 pair; f16mx8: fp16 + a remainder of one
        # bit, exact in block-scaled e4m3), the fine part is there in the mode that is about it and zero in every other
        for t, scale, fine in ((ref.x_norm, 1, mode in ("asplit", "arem")), (inp.w, cx.SW, mode in ("wsplit", "wrem"))):
            v = (t.double() / scale).float()
            assert torch.equal(v.double(), t.double() / scale)
            hi = v.to(torch.bfloat16).float()
            lo = (v - hi).to(torch.bfloat16).float()
            rem = v - v.to(torch.float16).float()
            if mode in ("int", "wsplit", "asplit"):
                assert torch.equal(hi + lo, v) and bool((lo != 0).any()) == fine
            if mode in ("int", "wrem", "arem"):
                assert bool((rem != 0).any()) == fine and set(rem.abs().unique().tolist()) <= {0.0, 2.0 ** -12}
            if not fine:
                assert torch.equal(v.to(torch.float16).float(), v) and torch.equal(v.to(torch.float8_e4m3fn).float(), v)
        if case.in_norm:
            assert bool((inp.mean != 0).all()) and set(inp.rstd2.tolist()) <= {1, 2, 4}
        if case.epi == "res":
            assert int(inp.res.abs().max()) <= 3
    # "wsplit": the lo plane is non-zero in 12 of the 21 values k + s 2^-9 of the integer range
    vals = torch.tensor([k + s * 2.0 ** -9 for k in range(-3, 4) for s in (-1, 0, 1)])
    hi = vals.to(torch.bfloat16).float()
    assert int(((vals - hi) != 0).sum()) == 12 and torch.equal(hi + (vals - hi).to(torch.bfloat16).float(), vals)


@pytest.mark.parametrize("case", cx.CASES, ids=[c.name for c in cx.CASES])
def test_row_selects_its_kernel_instance(case):
    assert case.precisions and case.alpha > 0
    info = KERNELS[case.kernel]
    if not case.refused:                 # a feature goes only on the kernels whose conv_select.KERNELS entry admits it
        assert info.stats or not case.stats
        assert info.in_norm or not case.in_norm
        assert info.roi or case.rect is None
        assert case.cout % 4 == 0 or (case.epi != "res" and not case.stats and not case.bias_map)
        assert not (case.in_norm and len(case.cin) == 2)
    if case.rect:
        y0, x0, rh, rw = case.rect
        ho, wo = cx.out_hw(case)
        assert 0 <= y0 and 0 <= x0 and rh > 0 and rw > 0 and y0 + rh <= ho and x0 + rw <= wo
    if len(case.cin) == 2:
        assert case.cin[0] % 32 == 0 and case.x2_off % 4 == 0 and case.x2_off > 0
    for precision in case.precisions:
        sel = cx.selection(case, precision)
        assert (sel.kernel, sel.tile_n) == (case.kernel, case.tile_n), (precision, sel)
        assert sel.precision == conv_select.PRECISION[precision], (precision, sel)          # (f16mx8 rows must not demote to bf16x3)
        assert sel.in_norm == case.in_norm
        if case.kernel == Kernel.GATHER:
            assert sel.tile_m == case.tile_m
        # ... and ops.conv_params derives the same layer from real operands (host tensors: the library is not loaded)
        dev, ops.DEV = ops.DEV, "cpu"
        mx, ops.MX_LAYERS = ops.MX_LAYERS, "all"
        try:
            pc = ops.pack_conv(torch.zeros(case.cout, sum(case.cin), *case.taps), None, stride=case.stride, flat_cs=case.flat_cs)
            n, h, w = case.nhw
            x = ops.Act(torch.zeros(1, case.flat_cs or ops._round_up(case.cin[0], 32)), n, h, w, case.cin[0])
            x2 = ops.Act(torch.zeros(1, 64), n, h, w, case.cin[1]) if len(case.cin) == 2 else None
            tiles, halo = cx.overrides(case)
            got = ops.select_conv(x, pc, epi=cx.EPI[case.epi], x2=x2, stats=(None, None) if case.stats else None, tiles=tiles,
                                  precision=precision, halo=halo, in_norm=case.in_norm, bias_map=True if case.bias_map else None)
        finally:
            ops.DEV, ops.MX_LAYERS = dev, mx
        assert got == sel, (precision, got, sel)
        assert (pc.cout_pad, pc.cin_pad, pc.out_hw(h, w)) == (cx.cout_pad(case), cx.cin_pad(case), cx.out_hw(case))


def test_table_covers_every_instance():
    have = {(c.kernel, c.tile_n, cx.selection(c, p).precision) for c in RUN for p in c.precisions}
    assert have >= set(COVERAGE), sorted(set(COVERAGE) - have)
    assert {(c.tile_m, c.tile_n) for c in RUN if c.kernel == Kernel.GATHER} == GATHER_TILES
    assert {c.kernel for c in RUN} == set(Kernel)
    # every feature on every kernel that admits it
    for kernel, info in KERNELS.items():
        rows = [c for c in RUN if c.kernel == kernel]
        assert {c.alpha for c in rows} > {1.0}, kernel
        assert any(c.co_off for c in rows) and any(c.epi == "relu" for c in rows) and any(c.epi == "res" for c in rows), kernel
        if kernel != Kernel.STEM:                                     # (the stem kernel takes no per-pixel bias, one source, 7x7)
            assert any(c.bias_map for c in rows), kernel
        if kernel not in (Kernel.STEM, Kernel.WINDOW_9X9):
            assert any(len(c.cin) == 2 for c in rows) and any(sum(c.cin) == 32 for c in rows) and any(sum(c.cin) == 96 for c in rows), kernel
            assert {64 if kernel != Kernel.REGB_4X16X128 and kernel != Kernel.GEMM_1X1 else 128} <= {c.cout for c in rows}, kernel
            assert any(c.cout % 4 for c in rows) and any(c.cout == 192 for c in rows), kernel
        assert any(c.stats for c in rows) == info.stats, kernel
        assert {c.in_norm for c in rows} == ({0, 1, 2} if info.in_norm else {0}), kernel
        assert any(c.rect for c in rows) == info.roi, kernel
        if info.tile not in (None, conv_select.RUNS_64, (9, 9)) and kernel != Kernel.STEM:
            assert {c.taps for c in rows} == set(conv_select.HALO_TAPS) and {c.nhw for c in rows} == {cx.H1, cx.H2}, kernel
    assert {c.taps for c in RUN if c.kernel == Kernel.GATHER and not c.flat_cs} == {(3, 3), (1, 5), (5, 1), (1, 1)}
    assert {(c.taps, c.flat_cs, c.stride) for c in RUN if c.kernel == Kernel.GATHER and c.flat_cs} == {((7, 7), 4, 1), ((7, 7), 4, 2), ((3, 3), 8, 1)}
    assert {(c.taps, c.stride) for c in RUN if c.kernel == Kernel.GATHER and c.stride == 2} >= {((3, 3), 2), ((1, 1), 2)}
    # the pairs: one per pair rule at least, both layers on the rule's kernel
    rules = {KERNELS[k].pair for k in Kernel} - {None}
    assert {rule for rule, _, _ in cx.PAIRS} == rules
    for rule, a, b in cx.PAIRS:
        a, b = cx.BY_NAME[a], cx.BY_NAME[b]
        assert a.kernel == b.kernel and KERNELS[a.kernel].pair == rule and not a.stats and not b.stats and a.precisions == b.precisions
        if rule != conv_select.PAIR_ANY:
            assert a.tile_n == b.tile_n
        if rule == conv_select.PAIR_SAME_TILES:
            assert a.tile_m == b.tile_m
        if rule == conv_select.PAIR_SAME_TAPS:
            assert a.taps == b.taps and a.taps != (1, 1)
    assert any(c.refused for c in cx.CASES) and all(len(c.refused) > 10 for c in cx.CASES if c.refused)


@pytest.mark.parametrize("case", RUN, ids=IDS)
def test_inputs_are_not_degenerate(case):
    """A kernel that drops a tap, drops a 32-channel chunk or pads one pixel off computes something else on these inputs."""
    inp, ref = cx.inputs(case, "int"), cx.reference(case, "int")
    kh, kw = case.taps
    for ky in range(kh):
        for kx in range(kw):
            w = inp.w.clone()
            w[:, :, ky, kx] = 0
            assert not torch.equal(cx.reference(case, "int", inp._replace(w=w)).out, ref.out), (ky, kx)
    cin = sum(case.cin)
    for c0 in range(0, cin, 32):
        w = inp.w.clone()
        w[:, c0:c0 + 32] = 0
        assert not torch.equal(cx.reference(case, "int", inp._replace(w=w)).out, ref.out), c0
    for shift in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        assert not torch.equal(cx.reference(case, "int", pad_shift=shift).out, ref.out), shift
    if case.in_norm:                     # padding before the normalisation instead of after it: (0 - mean) * rstd at the border
        x = cx.as_float(inp.x, cx.SA)
        xp = F.pad(x, (1, 1, 1, 1))
        xp = (xp - inp.mean.double().view(1, -1, 1, 1)) * (inp.rstd2.double() / 2).view(1, -1, 1, 1)
        xp = F.relu(xp) if case.in_norm == 2 else xp
        wrong = F.conv2d(xp, cx.as_float(inp.w, cx.SW))
        right = F.conv2d(ref.x_norm, cx.as_float(inp.w, cx.SW), padding=1)
        assert not torch.equal(wrong, right)


def test_modes_of_a_row():
    for case in RUN:
        want = ("int", "wsplit", "asplit") if set(case.precisions) & {"fp32", "bf16x3"} else ("int",)
        assert cx.all_modes(case) == want + (("wrem", "arem") if "f16mx8" in case.precisions else ())
        assert all(cx.modes(case, p) == ("int",) for p in case.precisions if p in ("bf16", "fp16"))


def test_a_moved_row_or_a_broken_bound_fails():
    """The checks above bite: a row made to select another kernel, or values past the bound, do not pass."""
    row = cx.BY_NAME["regb8_3x3_c32_o64"]._replace(kernel=Kernel.HALO_8X16, force=False)
    assert cx.selection(row, "bf16x3").kernel != row.kernel
    moved = cx.BY_NAME["gemm_1x1_c96_o256_m70"]._replace(cout=128)          # (no longer a 256-column layer: the gather kernel)
    assert cx.selection(moved, "bf16x3").kernel == Kernel.GATHER
    case = cx.BY_NAME["win_linear"]
    inp = cx.inputs(case, "int")
    big = inp._replace(x=inp.x * 64 + 1)                                    # (values up to 192 on a grid of 2^-10)
    assert cx.reference(case, "int", big).bound >= 2 ** 24
    stats = cx.BY_NAME["gather_3x3_stats"]
    inp = cx.inputs(stats, "int")
    assert cx.reference(stats, "int", inp._replace(x=inp.x * 64)).stat_bound >= 2 ** 24
