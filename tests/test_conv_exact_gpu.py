"""Every conv kernel instance against the integer convolution, bit for bit (the table and the reference: tests/conv_exact_cases.py;
why the values are exact: its docstring, checked by test_conv_exact_cpu.py).  One test per table row; the row's precisions and
value modes run inside it.  Zero tolerance: torch.equal on the whole output buffer, the sentinel around the written part included.
Run on the MI355X box: pytest -m gpu."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import conv_exact_cases as cx  # noqa: E402
from woft_amd import conv_select  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from woft_amd import _lib, ops as o
    _lib.load()
    assert cx.EPI == {"linear": _lib.EPI_LINEAR, "relu": _lib.EPI_RELU, "res": _lib.EPI_RELU_RES_RELU}
    return o


def _f32(t64):
    t = t64.float()
    assert torch.equal(t.double(), t64)                  # (the cast of an expected value is exact)
    return t


class Operands:
    """A row's device operands in one value mode: built once, shared by the row's precisions."""

    def __init__(self, ops, case, mode):
        inp = cx.inputs(case, mode)
        self.ref = cx.reference(case, mode)
        assert self.ref.bound < 2 ** 24 and (mode != "int" or self.ref.stat_bound < 2 ** 24)
        n, h, w = case.nhw
        x = _f32(cx.as_float(inp.x, cx.SA))
        self.pc = ops.pack_conv(_f32(cx.as_float(inp.w, cx.SW)), inp.bias.float(), stride=case.stride, flat_cs=case.flat_cs)
        self.kw = dict(co_off=case.co_off, epi=cx.EPI[case.epi], alpha=case.alpha)
        if len(case.cin) == 2:                           # the second source inside a wider tensor, other values around it
            c0, c1 = case.cin
            self.x = ops.act_from_nchw(x[:, :c0], cs=c0)
            t = torch.full((n * h * w, case.x2_off + c1 + 4), 5.0, device=DEV)
            t[:, case.x2_off:case.x2_off + c1] = x[:, c0:].permute(0, 2, 3, 1).reshape(n * h * w, c1).to(DEV)
            self.kw.update(x2=ops.Act(t, n, h, w, c1), c_split=c0, x2_off=case.x2_off)
        else:
            self.x = ops.act_from_nchw(x, cs=case.flat_cs or ops._round_up(case.cin[0], 32))
        if case.bias_map:
            self.kw["bias_map"] = ops.act_from_nchw(inp.bias_map.float())
        if case.epi == "res":
            self.kw["e0"] = ops.act_from_nchw(inp.res.float())
        if case.in_norm:
            self.kw.update(in_norm=case.in_norm, in_stats=(inp.mean.float().to(DEV), (inp.rstd2.float() / 2).to(DEV)))
        self.want = _f32(self.ref.buffer)


def _launch_args(ops, case, od, precision):
    """-> (params, output tensor, statistics tensors | None) of one launch, the output pre-filled with the sentinel."""
    n, (ho, wo) = case.nhw[0], cx.out_hw(case)
    out = torch.full((n * ho * wo + cx.TAIL_ROWS, cx.ldo(case)), cx.SENTINEL, device=DEV)
    sel = cx.selection(case, precision)
    stats = None
    if case.stats:
        stats = tuple(torch.zeros(2 * sel.m_tiles * od.pc.cout_pad + 64, device=DEV) for _ in range(2))
    tiles, halo = cx.overrides(case)
    p = ops.conv_params(od.x, od.pc, ops.Act(out, n, ho, wo, case.cout), tiles=tiles, halo=halo, precision=precision, stats=stats, **od.kw)
    assert (conv_select.Kernel(p.halo), p.tile_n, p.precision) == (case.kernel, case.tile_n, conv_select.PRECISION[precision]), \
        (p.halo, p.tile_n, p.precision)
    assert p.in_norm == case.in_norm and p._m_tiles == sel.m_tiles and p.cout_pad == sel.cout_pad
    if case.kernel == conv_select.Kernel.GATHER:
        assert p.tile_m == case.tile_m
    if case.rect:
        p.roi_y0, p.roi_x0, p.roi_h, p.roi_w = case.rect
    return p, out, stats


def _same(got, want, what):
    got = got.cpu()
    if torch.equal(got, want):
        return
    bad = (got != want) | (got.isnan() != want.isnan())
    rows, cols = bad.nonzero(as_tuple=True)
    r, c = int(rows[0]), int(cols[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} values differ from the integer reference ({len(set(rows.tolist()))} "
                         f"rows, {len(set(cols.tolist()))} columns); first at row {r}, column {c}: got {float(got[r, c])!r}, want "
                         f"{float(want[r, c])!r}; largest difference {float((got - want)[bad].abs().max()):.6g}")


def _check(case, od, mode, precision, p, out, stats):
    what = f"{case.name} {precision} {mode}"
    _same(out, od.want, what)
    if stats is not None and mode == "int":              # the 2 * m_tiles partial rows per channel, totalled as integers
        ld, rows = p.cout_pad, 2 * p._m_tiles
        for t, want, name in ((stats[0], od.ref.stat_sum, "sum y"), (stats[1], od.ref.stat_sq, "sum y^2")):
            t = t.cpu().double()
            assert bool((t[rows * ld:] == 0).all()), f"{what}: statistics written behind the launch's rows"
            tot = t[:rows * ld].reshape(rows, ld).sum(dim=0)
            assert torch.equal(tot[:case.cout], want), f"{what}: {name} differs, largest difference {float((tot[:case.cout] - want).abs().max())}"
            assert bool((tot[case.cout:] == 0).all()), f"{what}: {name} of padding columns"


@pytest.mark.parametrize("case", cx.CASES, ids=[c.name for c in cx.CASES])
def test_conv_is_the_integer_convolution(ops, monkeypatch, case):
    monkeypatch.setattr(ops, "MX_LAYERS", "all")         # f16mx8 on every multi-tap layer of the register-streamed kernel
    from woft_amd._lib import WoftHipError
    for mode in cx.all_modes(case):
        od = Operands(ops, case, mode)
        for precision in case.precisions:
            if mode not in cx.modes(case, precision):
                continue
            p, out, stats = _launch_args(ops, case, od, precision)
            if case.refused:                             # refused with WOFT_EINVAL, nothing launched
                with pytest.raises(WoftHipError):
                    ops.run_conv(p)
                torch.cuda.synchronize()
                assert bool((out == cx.SENTINEL).all()), (case.name, precision)
                continue
            ops.run_conv(p)
            torch.cuda.synchronize()
            _check(case, od, mode, precision, p, out, stats)


@pytest.mark.parametrize("rule,first,second", cx.PAIRS, ids=[f"{a}+{b}" for _, a, b in cx.PAIRS])
def test_pair_launch_is_the_integer_convolution(ops, monkeypatch, rule, first, second):
    """woft_conv2d_pair, one pair per pair rule of conv_select.KERNELS: both layers of the one launch against their own references,
    in either order of the two."""
    monkeypatch.setattr(ops, "MX_LAYERS", "all")
    a, b = cx.BY_NAME[first], cx.BY_NAME[second]
    assert conv_select.KERNELS[a.kernel].pair == rule
    for mode in cx.all_modes(a):
        oa, ob = Operands(ops, a, mode), Operands(ops, b, mode)
        for precision in a.precisions:
            if precision == "fp32" or mode not in cx.modes(a, precision):        # (the fp32 kernel takes one layer per launch)
                continue
            for swap in (False, True):
                pa, outa, _ = _launch_args(ops, a, oa, precision)
                pb, outb, _ = _launch_args(ops, b, ob, precision)
                assert ops.pair_ok(pa, pb) and ops.pair_ok(pb, pa)
                ops.run_conv_pair(*((pb, pa) if swap else (pa, pb)))
                torch.cuda.synchronize()
                _check(a, oa, mode, precision, pa, outa, None)
                _check(b, ob, mode, precision, pb, outb, None)
