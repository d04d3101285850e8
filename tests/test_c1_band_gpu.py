"""convc1 sampling the correlation band inside its own launch (woft_conv1x1_band), kernel level: band lookup with the samples
deferred + fallback + the fused launch against band lookup + fallback + woft_conv2d_pair on the same guarded buffers, bit for bit,
under both pre-fills -- c1, fl1, coordinates, the gather's outputs, the miss flags and the counter; guard columns and pad rows
untouched; and with the deferral no sample of a hit block makes the round trip through the lookup buffer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from woft_amd import _lib, ops  # noqa: E402
import lookup_cases as LC  # noqa: E402
from test_lookup_band_gpu import M0, _below, _expected_flags, _grid, _scene  # noqa: E402
from test_lookup_edges_gpu import FILLS, Guarded, _otf_params, _same_bits  # noqa: E402

# (band terms, conv precision): the engine's bf16x3, bf16 and fp16 modes
MODES = [(3, "bf16x3"), (1, "bf16"), (3, "fp16")]
_LAYERS = {}


def _layers():
    """convc1 (324 -> 256, 1x1) and convf1 (2 -> 128, 7x7 on the 4-channel flow rows), random weights, packed once."""
    if not _LAYERS:
        g = torch.Generator().manual_seed(11)
        _LAYERS["c1"] = ops.pack_conv(torch.randn(256, 324, 1, 1, generator=g) * 0.08, torch.randn(256, generator=g) * 0.1)
        _LAYERS["f1"] = ops.pack_conv(torch.randn(128, 2, 7, 7, generator=g) * 0.1, torch.randn(128, generator=g) * 0.1, flat_cs=4)
    return _LAYERS["c1"], _LAYERS["f1"]


def _run(s, coords, fused, fill, precision, fh=None, partner=True):
    """One iteration's lookup + convc1 (+ convf1) on guarded copies: the three existing launches, or the fused form.
    -> dict of arrays; "look" = the lookup buffer's rows."""
    h, w, k, r = s["h"], s["w"], s["k"], s["r"]
    P = h * w
    pc1, pcf = _layers()
    cg = Guarded(P, 2, 2, fill).put(coords)
    look = Guarded(P, 324, 352, fill)
    c1o, f1o = Guarded(P, 256, 264, fill), Guarded(P, 128, 136, fill)
    flow4 = Guarded(P, 4, 4, fill)
    p = _otf_params(s["f1s"], s["f2s"], s["dims"], h, w, k, cg.view, look.view, r, s["terms"], 4)
    res = dict(c1=c1o, coords=cg)
    if fh is not None:
        part, n_planes, bias = fh
        delta, cat = Guarded(P, 2, 4, fill), Guarded(P, 2, 12, fill, col0=6)
        p.fh_part, p.fh_bias, p.fh_delta = part.data_ptr(), bias.data_ptr(), delta.ptr()
        p.fh_flow4, p.fh_flow_cat = flow4.ptr(), cat.ptr()
        p.fh_planes, p.fh_ld, p.fh_ld_delta, p.fh_ld_cat = n_planes, part.shape[1], 4, 12
        res.update(delta=delta, cat=cat)
    else:                                                # (no gather: convf1 reads the flow the caller supplies)
        f = np.zeros((P, 4), np.float32)
        f[:, :2] = np.asarray(coords, np.float32) - _grid(h, w)
        flow4.put(f)
    res.update(flow4=flow4)
    c1 = ops.conv_params(ops.Act(look.view, 1, h, w, 324), pc1, ops.Act(c1o.view, 1, h, w, 256), epi=_lib.EPI_RELU, precision=precision)
    f1 = None
    if partner:
        f1 = ops.conv_params(ops.Act(flow4.view, 1, h, w, 4), pcf, ops.Act(f1o.view, 1, h, w, 128), epi=_lib.EPI_RELU,
                             precision=precision)
        assert ops.pair_ok(c1, f1)
        res.update(fl1=f1o)
    assert (c1.halo, c1.cin_pad, c1.cout_pad, c1.tile_n) == (16, 352, 256, 256)
    miss = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    bp = ops.make_lookup_band_params(p, s["band"], miss, count)
    bp.defer_samples = 1 if fused else 0
    ops.run_lookup_band(bp)
    fb = ops.copy_params(p)
    fb.fh_part, fb.need = None, miss.data_ptr()
    ops.run_lookup_otf(fb)
    if fused:
        ops.run_conv1x1_band(c1, f1, bp)
    elif partner:
        ops.run_conv_pair(c1, f1)
    else:
        ops.run_conv(c1)
    torch.cuda.synchronize()
    out = {n: g.numpy() for n, g in res.items()}                 # (asserts the guards of every buffer)
    if not partner:
        out["fl1_untouched"] = f1o.numpy()
    out.update(look=look.numpy(), miss=miss.cpu().numpy(), count=int(count.item()))
    return out


def _compare(s, coords, precision, expect_misses=None, **kw):
    """Fused form == three-launch form under both pre-fills; the lookup buffer keeps its pre-fill where blocks hit."""
    h, w = s["h"], s["w"]
    for fill in FILLS:
        a, b = _run(s, coords, False, fill, precision, **kw), _run(s, coords, True, fill, precision, **kw)
        for name in a:
            if name == "look":
                continue
            if name in ("miss", "count"):
                assert np.array_equal(a[name], b[name]), name
            else:
                _same_bits(a[name], b[name], name)
        assert np.isfinite(b["c1"]).all() and (b["c1"] > 0).any() and not (b["c1"] == np.float32(fill)).any()
        flags, n = _expected_flags(s, b["coords"])
        assert np.array_equal(b["miss"], flags) and b["count"] == n
        missed = flags.astype(bool)
        assert (b["look"][~missed] == np.float32(fill)).all(), "a sample of a hit block went through the lookup buffer"
        _same_bits(a["look"][missed], b["look"][missed], "rows of missed blocks")
        assert not (a["look"] == np.float32(fill)).any()
        if "fl1_untouched" in b:
            assert (b["fl1_untouched"] == np.float32(fill)).all()
    if expect_misses is not None:
        assert n == expect_misses, (n, expect_misses)
    return b


def _fields(h, w):
    g = _grid(h, w)
    nb = len(LC.blocks(h, w))
    wave = np.stack([0.3 + 0.2 * np.sin(g[:, 1] * 0.7), -0.45 + 0.25 * np.cos(g[:, 0] * 0.5)], 1).astype(np.float32)
    return (("identity", g, 0), ("smooth", g + wave, 0), ("-m0", g - np.float32(M0), 0),
            ("below m0 + 1", _below(g + np.float32(M0 + 1)), 0), ("m0 + 1", g + np.float32(M0 + 1), nb))


@pytest.mark.parametrize("terms,precision", MODES)
@pytest.mark.parametrize("h,w", [(17, 25), (9, 11), (8, 8)])
def test_fused_launch_equals_the_three_launches(h, w, terms, precision):
    """Identity, a smooth sub-cell field, the last hits on both sides (-m_0, just below m_0 + 1) and m_0 + 1, where every block
    misses and the conv reads only rows the fallback wrote."""
    s = _scene(h, w, 256, terms)
    for name, c, misses in _fields(h, w):
        _compare(s, np.ascontiguousarray(c, np.float32), precision, expect_misses=misses)


@pytest.mark.parametrize("terms,precision", MODES)
@pytest.mark.parametrize("axis,sign", [(0, 1), (1, -1)])
def test_hit_and_missed_blocks_in_one_launch(terms, precision, axis, sign):
    """One pixel of block (1, 1) of 17 x 25 looks one cell beyond the band: that block takes its rows from the fallback, its
    neighbours sample the band, in the same launch."""
    h, w = 17, 25
    s = _scene(h, w, 256, terms)
    c = _grid(h, w) + np.float32(0.25)
    i = 10 * w + 11
    c[i, axis] = (np.float32(i % w if axis == 0 else i // w) + (np.float32(M0 + 1) if sign > 0 else np.float32(-M0 - 0.5)))
    b = _compare(s, c, precision, expect_misses=1)
    flags = b["miss"].reshape(h, w)
    assert flags[8:16, 8:16].all() and flags.sum() == 64


@pytest.mark.parametrize("terms,precision", MODES)
@pytest.mark.parametrize("scale,misses", [(0.02, False), (3.0, True)])
def test_with_the_folded_gather(terms, precision, scale, misses):
    """The lookup launch carries the folded flow-head gather (its stores stay there: convf1 reads the flow4 it writes); small
    updates (all hits) and updates of several cells (hit and missed blocks)."""
    h, w, n_planes = 17, 25, 2
    s = _scene(h, w, 256, terms)
    P = h * w
    g = torch.Generator().manual_seed(5)
    part = (torch.randn(n_planes * P, 20, generator=g) * scale).cuda()
    bias = torch.tensor([0.125, -0.25], device="cuda")
    c = _grid(h, w) + np.float32(0.25)
    b = _compare(s, c, precision, fh=(part, n_planes, bias))
    assert (b["count"] > 0) == misses
    assert np.array_equal(b["coords"], c + b["delta"])


@pytest.mark.parametrize("terms,precision", MODES)
def test_without_a_partner_layer(terms, precision):
    """convc1 alone (f1 = NULL): the smooth field and the mixed hit / miss field; convf1's output is never written."""
    h, w = 17, 25
    s = _scene(h, w, 256, terms)
    _compare(s, np.ascontiguousarray(_fields(h, w)[1][1], np.float32), precision, expect_misses=0, partner=False)
    c = _grid(h, w) + np.float32(0.25)
    c[10 * w + 11, 0] = np.float32(11 + M0 + 1)
    _compare(s, c, precision, expect_misses=1, partner=False)
