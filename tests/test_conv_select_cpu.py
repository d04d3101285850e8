"""The conv kernel selection against a record of the commit before it was last touched (tests/golden/conv_select.npz; grid and
row format: tests/conv_select_cases.py).  No GPU: conv_params reads geometry and addresses only, conv_select.select() integers."""
import re
from pathlib import Path

import numpy as np
import pytest

import conv_select_cases as grid
from woft_amd import conv_select, ops
from woft_amd.conv_select import F16MX8, BF16X3, Kernel

N_ROWS, N_PAIRS = 68150, 420500          # 58 layers x (25 maps x 5 precisions on the plain set + 6 maps x 5 x 30 other sets / switches)
COL = {name: k for k, name in enumerate(grid.OUTCOME)}


@pytest.fixture(scope="module")
def recorded():
    with np.load(grid.FIXTURE) as f:
        return dict(rows=f["rows"].astype(np.int64), pairs=np.unpackbits(f["pairs"])[:int(f["n_pairs"])], raised=list(f["raised"]))


@pytest.fixture(scope="module")
def layers():
    return grid.layers()


@pytest.fixture(scope="module")
def cases(layers):
    return list(grid.cases(len(layers)))


def _describe(k, cases, layers):
    c = cases[k]
    return f"row {k}: {layers[c.layer][0]} on {grid.MAPS[c.map]} {c.precision} option {c.option} switch {c.switch}"


def test_conv_params_reproduces_every_row(recorded, layers, cases):
    """(a) and the pair verdicts: every struct conv_params fills is the recorded one, field for field (CRC32 of its canonical
    form), every call that raised still raises the same exception type, pair_ok answers as recorded."""
    raised, sample = list(recorded["raised"]), []
    rows, pairs = grid.run(layers, raised, visit=lambda k, case, p: k % 997 == 0 and sample.append(
        grid.canonical(p) == grid.canonical_reference(p)))
    assert len(cases) == len(rows) == len(recorded["rows"]) == N_ROWS
    assert raised == recorded["raised"]
    bad = np.nonzero((rows != recorded["rows"]).any(axis=1))[0]
    assert bad.size == 0, (f"{bad.size} rows differ; first: {_describe(bad[0], cases, layers)}\n  {grid.OUTCOME}\n"
                           f"  recorded {recorded['rows'][bad[0]].tolist()}\n  now      {rows[bad[0]].tolist()}")
    assert len(sample) > 50 and all(sample)                  # the fast canonical form is launch_trace.LibProxy._struct's
    assert pairs.size == recorded["pairs"].size == N_PAIRS
    assert np.array_equal(pairs, recorded["pairs"])


def _layer(case, pc):
    """The selection's inputs of a case, from integers alone."""
    n, h, w = grid.MAPS[case.map]
    ho, wo = pc.out_hw(h, w)
    name, val = case.option
    return conv_select.Layer(n, h, w, ho, wo, pc.taps_y, pc.taps_x, pc.stride, pc.pad_y, pc.pad_x, pc.cin_pad,
                             (pc.cout + 1) // 2 if name == "cout" else pc.cout, pc.cout_pad, pc.flat,
                             pc.flat_cs if pc.flat else pc.cin_pad, name == "x2", name == "stats", val if name == "in_norm" else 0,
                             name == "bias_map", name == "wh0", 9 if name == "flowhead" else 0)


def test_select_alone_gives_every_outcome(recorded, layers, cases):
    """(b) conv_select.select() on integers and flags, without a tensor, gives every non-raising row's outcome."""
    want = recorded["rows"]
    for k, case in enumerate(cases):
        if want[k, COL["raised"]]:
            continue
        sw = conv_select.Switches()
        if case.switch is not None:
            sw = sw._replace(**{"mx_zr" if case.switch[0] == "WOFT_MX_ZR" else case.switch[0].lower(): case.switch[1]}) \
                if case.switch[0] != "SLOW_GATES" else sw
        name, val = case.option
        got = conv_select.select(_layer(case, layers[case.layer][1]), ops.PRECISION[case.precision], sw,
                                 tiles=val if name == "tiles" else None, halo=val if name == "halo" else None)
        assert tuple(int(v) for v in got) == tuple(want[k, :7]), _describe(k, cases, layers)


def test_grid_coverage(recorded, layers, cases):
    """(c) the grid reaches what the selection can do: a shrunken grid cannot pass silently."""
    rows = recorded["rows"]
    ok = rows[:, COL["raised"]] == 0
    kernel, tile_n, prec, in_norm = (rows[:, COL[c]] for c in ("kernel", "tile_n", "precision", "in_norm"))
    assert set(kernel[ok]) == {int(k) for k in Kernel}
    assert {(k, t) for k in (Kernel.HALO_8X16, Kernel.HALO_4X16, Kernel.REGB_8X16) for t in (64, 128)} <= set(zip(kernel[ok], tile_n[ok]))
    asked_mx = np.array([c.precision == "f16mx8" for c in cases]) & ok
    regb = np.isin(kernel, conv_select.REGB)
    assert (asked_mx & (prec == F16MX8)).any()
    assert (asked_mx & (prec == BF16X3) & ~regb).any()                      # demoted: the kernel has no f16mx8 instance
    assert (asked_mx & (prec == BF16X3) & regb).any()                       # demoted: a layer it measured slower on
    # under f16mx8 an 8x16 x 128-column 1x5 / 5x1 layer is moved to the 4x16 x 128 layout: the same case in bf16x3 stays
    at = {(c.layer, c.map, c.option, c.switch, c.precision): k for k, c in enumerate(cases)}
    moved = [k for k, c in enumerate(cases) if asked_mx[k] and prec[k] == F16MX8 and kernel[k] == Kernel.REGB_4X16X128
             and kernel[at[(c.layer, c.map, c.option, c.switch, "bf16x3")]] == Kernel.REGB_8X16]
    assert moved
    asked_norm = np.array([c.option[0] == "in_norm" for c in cases]) & ok
    assert (asked_norm & (in_norm == 0)).any() and (asked_norm & (in_norm == 1)).any() and (asked_norm & (in_norm == 2)).any()
    assert (~ok).any() and 0 < recorded["pairs"].sum() < recorded["pairs"].size


def test_no_kernel_number_outside_the_selection_module():
    """The kernels' numbers are compared by name: only conv_select.py knows what a value of woft_conv_params.halo means."""
    src = Path(ops.__file__).parent
    hits = [f"{p.name}:{n}" for p in sorted(src.glob("*.py")) if p.name != "conv_select.py"
            for n, line in enumerate(p.read_text().splitlines(), 1) if re.search(r"halo\s*(==|!=|in\s*\()", line)]
    assert not hits, hits
