"""The correlation band (woft_corr_band_build) and the lookup that samples from it (woft_corr_lookup_band + the volume-free
lookup on the blocks it flags): every comparison is bit for bit.

Band cells: against the volume woft_corr_gemm_bf16 builds from the same row-major operands, zeros beyond the map.  Lookup: band
lookup + fallback against the plain woft_corr_lookup_otf launch on the same inputs -- outputs, coordinates and flow operands --
with the miss flags and the miss counter checked against the host mirror of the hit rule (ops.band_hit)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from woft_amd import _lib, ops  # noqa: E402
import lookup_cases as LC  # noqa: E402
from test_lookup_edges_gpu import FILLS, Guarded, _nout, _otf_params, _same_bits  # noqa: E402

M0 = ops.BAND_M0


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _operand(t, terms):
    k = t.shape[1]
    if terms == 3:
        o = torch.zeros(t.shape[0], 2 * k, dtype=torch.bfloat16, device="cuda")
        ops.split_bf16_lines(t.contiguous(), o)
    else:
        o = torch.zeros(t.shape[0], k, dtype=torch.bfloat16, device="cuda")
        ops.split_bf16(t.contiguous(), o, None)
    return o


_CACHE = {}


def _scene(h, w, k, terms):
    """Random maps, their pooled levels, the operands of `terms`, and the band built from them (once per setting)."""
    key = (h, w, k, terms)
    if key not in _CACHE:
        r = 4 if k == 256 else 3
        g = torch.Generator().manual_seed(7 * h + 13 * w + k + terms)
        f1 = (torch.rand(1, k, h, w, generator=g) * 2 - 1)
        f2 = (torch.rand(1, k, h, w, generator=g) * 2 - 1)
        a1, cur = ops.act_from_nchw(f1), ops.act_from_nchw(f2)
        rows1 = torch.zeros(ops._round_up(h * w, 128), k, device="cuda")
        rows1[:h * w] = a1.t
        f1s = _operand(rows1, terms)
        f2s, dims = [], []
        for l in range(4):
            rows = torch.zeros(ops._round_up(cur.h * cur.w, 128), k, device="cuda")
            rows[:cur.h * cur.w] = cur.t[:, :k]
            f2s.append(_operand(rows, terms))
            dims.append((cur.h, cur.w))
            if l < 3:
                nxt = ops.new_act(1, max(cur.h // 2, 1), max(cur.w // 2, 1), k)
                ops.avgpool2(cur, nxt)
                cur = nxt
        assert dims == LC.level_dims(h, w)
        rows_pp = ops.band_geometry(r, 4)[3]
        band = torch.full((h * w, rows_pp, ops.BAND_LD), float("nan"), device="cuda")
        miss = torch.full((h * w,), -7, dtype=torch.int32, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        dummy = torch.zeros(h * w, 2, device="cuda")
        otf = ops.make_lookup_otf_params(f1s, f2s, dims, h, w, k, dummy, dummy, r, terms)
        ops.run_band_build(ops.make_lookup_band_params(otf, band, miss, count))
        torch.cuda.synchronize()
        _CACHE[key] = dict(f1s=f1s, f2s=f2s, dims=dims, band=band, r=r, k=k, terms=terms, h=h, w=w)
    return _CACHE[key]


# ---- band cells -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,terms", [(256, 3), (256, 1), (128, 3), (128, 1)])
def test_band_cells_equal_the_correlation_gemm(k, terms):
    """17 x 25 (ragged blocks; levels 8 x 12, 4 x 6, 2 x 3): every stored cell is the entry of the woft_corr_gemm_bf16 volume for that
    pair, cells beyond the map and the padding entries of a row are exact zeros.  Nothing of the buffer keeps its NaN pre-fill."""
    h, w = 17, 25
    s = _scene(h, w, k, terms)
    r, P = s["r"], h * w
    m, wl, off, rows = ops.band_geometry(r, 4)
    lib_m, lib_w, lib_off = (np.zeros(4, np.int32) for _ in range(3))
    i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert _lib.load().woft_corr_band_geometry(r, 4, i32p(lib_m), i32p(lib_w), i32p(lib_off)) == rows
    assert (list(lib_m), list(lib_w), list(lib_off)) == (m, wl, off)
    band = s["band"].cpu().numpy()
    assert np.isfinite(band).all()
    ys, xs = np.divmod(np.arange(P), w)
    for l, (hl, wl_map) in enumerate(s["dims"]):
        n = hl * wl_map
        vol = torch.zeros(P, ops._round_up(n, 128), device="cuda")
        # (the GEMM takes column counts in multiples of 4: the operand's rows beyond the map are zero)
        ops.corr_gemm_bf16(s["f1s"], s["f2s"][l], P, ops._round_up(n, 4), 1.0 / math.sqrt(k), vol, terms)
        torch.cuda.synchronize()
        vol = vol[:, :n].cpu().numpy().reshape(P, hl, wl_map)
        want = np.zeros((P, wl[l], ops.BAND_LD), np.float32)
        for bx in range(wl[l]):
            for by in range(wl[l]):
                qx, qy = (xs >> l) - r - m[l] + bx, (ys >> l) - r - m[l] + by
                inside = (qx >= 0) & (qx < wl_map) & (qy >= 0) & (qy < hl)
                want[inside, bx, by] = vol[np.nonzero(inside)[0], qy[inside], qx[inside]]
        got = band[:, off[l]:off[l] + wl[l]]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (l, int((got != want).sum()))
        assert (want != 0).any()


# ---- lookups --------------------------------------------------------------------------------------------------------------------
def _grid(h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.float32)


def _expected_flags(s, coords, launched=None):
    """Miss flags and missed-block count by the host mirror of the hit rule (launched: bool per block, default all)."""
    h, w = s["h"], s["w"]
    flags, n = np.zeros((h, w), np.int32), 0
    for by, bx in LC.blocks(h, w):
        if launched is not None and not launched[(by, bx)]:
            continue
        pix = [(y, x) for y in range(8 * by, min(8 * by + 8, h)) for x in range(8 * bx, min(8 * bx + 8, w))]
        if not all(ops.band_hit(float(coords[y * w + x, 0]), float(coords[y * w + x, 1]), x, y, 4) for y, x in pix):
            flags[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = 1
            n += 1
    return flags.reshape(-1), n


def _run(s, coords, band_path, fill, need=None, rects=None, fh=None):
    """One lookup on guarded copies of the buffers: the plain volume-free launch, or band lookup + fallback.
    -> dict(out, coords[, delta, flow4, cat], miss, count)."""
    h, w, k, r = s["h"], s["w"], s["k"], s["r"]
    P = h * w
    cg = Guarded(P, 2, 2, fill).put(coords)
    out = Guarded(P, _nout(4, r), _nout(4, r) + 28, fill)
    p = _otf_params(s["f1s"], s["f2s"], s["dims"], h, w, k, cg.view, out.view, r, s["terms"], 4)
    if need is not None:
        p.need = need.data_ptr()
    if rects is not None:
        (p.roi_y0, p.roi_x0, p.roi_h, p.roi_w), (p.smp_y0, p.smp_x0, p.smp_h, p.smp_w) = rects
    res = {}
    if fh is not None:
        part, n_planes, bias = fh
        delta, flow4, cat = Guarded(P, 2, 4, fill), Guarded(P, 4, 4, fill), Guarded(P, 2, 12, fill, col0=6)
        p.fh_part, p.fh_bias, p.fh_delta = part.data_ptr(), bias.data_ptr(), delta.ptr()
        p.fh_flow4, p.fh_flow_cat = flow4.ptr(), cat.ptr()
        p.fh_planes, p.fh_ld, p.fh_ld_delta, p.fh_ld_cat = n_planes, part.shape[1], 4, 12
        res.update(delta=delta, flow4=flow4, cat=cat)
    miss = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    if band_path:
        bp = ops.make_lookup_band_params(p, s["band"], miss, count)
        ops.run_lookup_band(bp)
        fb = ops.copy_params(p)
        fb.fh_part, fb.need = None, miss.data_ptr()
        ops.run_lookup_otf(fb)
    else:
        ops.run_lookup_otf(p)
    torch.cuda.synchronize()
    res = {n: g.numpy() for n, g in res.items()}
    res.update(out=out.numpy(), coords=cg.numpy(), miss=miss.cpu().numpy(), count=int(count.item()))
    return res


def _compare(s, coords, expect_misses=None, **kw):
    """Band path == plain path under both pre-fills; flags and counter as the host mirror says.  -> the band path's result."""
    for fill in FILLS:
        a, b = _run(s, coords, False, fill, **kw), _run(s, coords, True, fill, **kw)
        for name in a:
            if name not in ("miss", "count"):
                _same_bits(a[name], b[name], name)
    flags, n = _expected_flags(s, b["coords"])
    if kw.get("need") is None and kw.get("rects") is None:
        assert np.array_equal(b["miss"], flags) and b["count"] == n
    if expect_misses is not None:
        assert b["count"] == expect_misses, (b["count"], expect_misses)
    return b


def _below(a):
    return np.nextafter(np.asarray(a, np.float32), np.float32(-np.inf))


@pytest.mark.parametrize("h,w,k,terms", [(17, 25, 256, 3), (17, 25, 256, 1), (17, 25, 128, 3), (9, 11, 256, 3), (8, 8, 256, 3)])
def test_band_lookup_equals_the_volume_free_lookup(h, w, k, terms):
    """Identity (windows hang over every map border, level 3 is smaller than a window), a smooth sub-cell flow, the displacements
    -m_0 exactly and just below +m_0, and the true last hit on the positive side, just below m_0 + 1 (floor(coords) = p + m_0):
    all of them hit everywhere.  One float below -m_0 and m_0 + 1 exactly: every block misses, the fallback computes all."""
    s = _scene(h, w, k, terms)
    g = _grid(h, w)
    nb = len(LC.blocks(h, w))
    wave = np.stack([0.3 + 0.2 * np.sin(g[:, 1] * 0.7), -0.45 + 0.25 * np.cos(g[:, 0] * 0.5)], 1).astype(np.float32)
    for name, c, misses in (("identity", g, 0), ("smooth", g + wave, 0), ("-m0", g - np.float32(M0), 0),
                            ("below +m0", _below(g + np.float32(M0)), 0), ("below m0 + 1", _below(g + np.float32(M0 + 1)), 0),
                            ("below -m0", _below(g - np.float32(M0)), nb), ("m0 + 1", g + np.float32(M0 + 1), nb)):
        _compare(s, np.ascontiguousarray(c, np.float32), expect_misses=misses)


@pytest.mark.parametrize("axis,sign", [(0, -1), (0, 1), (1, -1), (1, 1)])
def test_one_pixel_beyond_the_band_flags_its_block_alone(axis, sign):
    """One pixel of block (1, 1) looks one cell beyond the band in one direction: that block is flagged (all its pixels) and
    counted, its neighbours are hits, and the outputs are the volume-free lookup's."""
    h, w = 17, 25
    s = _scene(h, w, 256, 3)
    c = _grid(h, w) + np.float32(0.25)
    i = 10 * w + 11
    c[i, axis] = (np.float32(i % w if axis == 0 else i // w) + (np.float32(M0 + 1) if sign > 0 else np.float32(-M0 - 0.5)))
    b = _compare(s, c, expect_misses=1)
    flags = b["miss"].reshape(h, w)
    assert flags[8:16, 8:16].all() and flags.sum() == 64


def test_need_subset_leaves_other_rows_untouched():
    """With a `need` map: blocks nobody needs keep their pre-fill and are flagged 0 (one of them would miss: it is not counted); a
    needed block that misses is computed by the fallback."""
    h, w = 17, 25
    s = _scene(h, w, 256, 3)
    c = _grid(h, w) + np.float32(0.25)
    c[9 * w + 3, 0] += np.float32(6)                     # block (1, 0): needed, misses
    c[2 * w + 18, 1] -= np.float32(6)                    # block (0, 2): not needed, would miss
    need = torch.zeros(h, w, dtype=torch.int32, device="cuda")
    need[16, 24], need[9, 3], need[12, 12] = 1, 7, 1     # blocks (2, 3), (1, 0), (1, 1)
    wanted = np.zeros((h, w), bool)
    wanted[16:, 24:], wanted[8:16, 0:16] = True, True
    wanted = wanted.reshape(-1)
    for fill in FILLS:
        a, b = _run(s, c, False, fill, need=need), _run(s, c, True, fill, need=need)
        _same_bits(a["out"], b["out"], "out")
        assert (b["out"][~wanted] == np.float32(fill)).all() and not (b["out"][wanted] == np.float32(fill)).any()
        flags = b["miss"].reshape(h, w)
        assert b["count"] == 1 and flags[8:16, 0:8].all() and flags.sum() == 64


def test_rectangles_leave_rows_outside_untouched():
    """roi_* = blocks (1..2, 1..2), smp_* = block (1, 2) only: rows outside the sampled block keep their pre-fill, the flags of
    blocks that were not launched are not written, launched blocks without samples are flagged 0."""
    h, w = 17, 25
    s = _scene(h, w, 256, 3)
    rects = ((8, 8, 9, 10), (8, 16, 8, 8))
    for shift, misses in ((np.float32(0.25), 0), (np.float32(M0 + 1.5), 1)):
        c = _grid(h, w) + shift
        for fill in FILLS:
            a, b = _run(s, c, False, fill, rects=rects), _run(s, c, True, fill, rects=rects)
            _same_bits(a["out"], b["out"], "out")
            sampled = np.zeros((h, w), bool)
            sampled[8:16, 16:24] = True
            assert (b["out"][~sampled.reshape(-1)] == np.float32(fill)).all()
            assert not (b["out"][sampled.reshape(-1)] == np.float32(fill)).any()
            flags = b["miss"].reshape(h, w)
            launched = np.zeros((h, w), bool)
            launched[8:, 8:24] = True
            assert (flags[~launched] == -7).all() and b["count"] == misses
            assert (flags[sampled] == misses).all() and (flags[launched & ~sampled] == 0).all()


@pytest.mark.parametrize("scale,misses", [(0.02, False), (3.0, True)])
def test_folded_gather_equals_the_volume_free_launch(scale, misses):
    """The band lookup with fh_part: coords, fh_delta, fh_flow4, fh_flow_cat and the samples equal those of the volume-free
    launch with fh_part -- with small updates (all hits) and with updates of several cells (misses: the fallback reads the
    coordinates the band launch wrote)."""
    h, w, n_planes = 17, 25, 2
    s = _scene(h, w, 256, 3)
    P = h * w
    g = torch.Generator().manual_seed(5)
    part = (torch.randn(n_planes * P, 20, generator=g) * scale).cuda()
    bias = torch.tensor([0.125, -0.25], device="cuda")
    c = _grid(h, w) + np.float32(0.25)
    b = _compare(s, c, fh=(part, n_planes, bias))
    assert (b["count"] > 0) == misses
    assert np.array_equal(b["coords"], c + b["delta"])
