"""The correlation lookups, the folded flow-head gather and the convex upsampling against float64 references at their edges.

woft_corr_lookup (volume) and woft_corr_lookup_otf (volume-free) are held to fp64_refs.lookup64, the lookup written in pixel
coordinates in numpy float64: bit for bit where the data makes every fp32 operation exact (lookup_cases: integer planes,
integer features, coordinates on multiples of 1/4), within fp64_refs.LOOKUP_BAND times the largest tap elsewhere, exact zeros
off the map.  The coordinate lists put every window edge, map edge, tile phase, clamp and one-float-off-an-integer case into
each level; tests/test_lookup_edges_cpu.py proves that coverage and -- by a host restatement of the kernels' index arithmetic
-- that none of the lists, the wild and non-finite ones included, makes a kernel address anything outside its level.  The
folded gather (woft_lookup_otf_params.fh_*) is held to the two-launch path bit for bit and to flow_head_gather64 within the
fixed-order summation bound.  Every output is a view into a sentinel buffer with guard rows and columns around it and runs
under two different pre-fills: the results must agree (every element was written) and the guards must survive."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from woft_amd import _lib, ops  # noqa: E402
import fp64_refs as R  # noqa: E402
import lookup_cases as LC  # noqa: E402
from test_kernels_gpu import _build_pyramid_gpu  # noqa: E402

GR = 3                               # guard rows before and after
FILLS = (77.0, -178.5)
EINVAL = -1


class Guarded:
    """A float32 output of `rows` x `cols` inside a (GR + rows + GR) x ld buffer pre-filled with `fill`, starting at column
    `col0` of its rows: guard rows on both sides, guard columns on both sides of the output's own."""

    def __init__(self, rows, cols, ld, fill, col0=0):
        assert col0 + cols <= ld
        self.rows, self.cols, self.ld, self.fill, self.col0 = rows, cols, ld, fill, col0
        self.buf = torch.full((GR + rows + GR, ld), fill, dtype=torch.float32, device="cuda")
        self.view = self.buf[GR:GR + rows, col0:]                          # (rows, ld - col0), row stride ld

    def ptr(self):
        return self.view.data_ptr()

    def put(self, a):
        self.buf[GR:GR + self.rows, self.col0:self.col0 + self.cols] = torch.as_tensor(a, dtype=torch.float32).cuda()
        return self

    def numpy(self, cols=None):
        """The output's first `cols` columns (all by default), after asserting that nothing around them was written."""
        cols = self.cols if cols is None else cols
        b = self.buf.cpu().numpy()
        own = np.zeros(b.shape, bool)
        own[GR:GR + self.rows, self.col0:self.col0 + cols] = True
        assert (b[~own] == np.float32(self.fill)).all(), "guard elements overwritten"
        return b[own].reshape(self.rows, cols).copy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b, what=""):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    a, b = np.where(a == 0, np.float32(0), a), np.where(b == 0, np.float32(0), b)          # (+0 and -0: the same value)
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), \
        (what, int((_bits(a) != _bits(b)).sum()), np.argwhere(_bits(a) != _bits(b))[:4].tolist())


def _in_band(got, want, m, what=""):
    err = np.abs(np.asarray(got, np.float64) - want)
    bad = ~(err <= R.LOOKUP_BAND * m)
    worst = float((err[m > 0] / m[m > 0]).max() / R.U32) if (m > 0).any() else 0.0
    print(f"LOOKUP {what}: {got.size} samples, largest error {worst:.2f} units of 2^-24 M, outside the band {int(bad.sum())}")
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _nout(levels, r):
    return levels * (2 * r + 1) ** 2


# ---- the volume lookup ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiled(h, w, bf16):
    planes = LC.volume_planes(h, w)
    dt = torch.bfloat16 if bf16 else torch.float32
    return [ops.tile_planes(torch.from_numpy(np.array(p)).to(dt).cuda()) for p in planes], LC.level_dims(h, w)


def _volume(vols, dims, coords, r, levels=4, extra=0):
    """woft_corr_lookup of `levels` levels into guarded outputs with ldo = the channel count + extra, under both pre-fills."""
    cg = torch.from_numpy(np.ascontiguousarray(coords, np.float32)).cuda()
    outs = []
    for fill in FILLS:
        g = Guarded(len(coords), _nout(levels, r), _nout(levels, r) + extra, fill)
        ops.run_lookup(ops.make_lookup_params(vols[:levels], dims[:levels], cg, g.view, r))
        torch.cuda.synchronize()
        outs.append(g.numpy())
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "the two pre-fills disagree: an element was not written"
    return outs[0]


VOLUME_SETTINGS = [(bf16, r, levels, extra) for bf16 in (False, True) for r, levels, extra in
                   ((4, 4, 0), (4, 4, 28), (3, 4, 0), (3, 4, 12), (4, 3, 5), (4, 1, 7), (4, 1, 0))]


@pytest.mark.parametrize("bf16,r,levels,extra", VOLUME_SETTINGS)
@pytest.mark.parametrize("h,w", LC.MAPS)
def test_volume_lookup_against_fp64(h, w, bf16, r, levels, extra):
    """`exact`: bit-equal to lookup64; `band`: within LOOKUP_BAND M, zero violations; `far`: exact zeros; `outlier`: bit-equal
    (its coordinates are multiples of 1/4) with all-zero rows at the far pixels.  fp32 and bf16-storage volumes, both radii,
    fewer levels than 4 (the tail loop of the 17 samples beyond lane 63 must stop at the right level: the channels of the
    levels not asked for are guard columns here), ldo equal to the channel count and larger."""
    vols, dims = _tiled(h, w, bf16)
    planes, P, n = LC.volume_planes(h, w)[:levels], h * w, _nout(levels, r)
    for k, (c, used) in enumerate(LC.launches(LC.exact(h, w, r), P)):
        want, _ = R.lookup64(planes, c, r)
        _same_bits(_volume(vols, dims, c, r, levels, extra), want, f"exact[{k}]")
    for k, (c, used) in enumerate(LC.launches(LC.band(h, w, r), P)):
        want, m = R.lookup64(planes, c, r)
        _in_band(_volume(vols, dims, c, r, levels, extra), want, m, f"volume band[{k}] {h}x{w} bf16={bf16} r={r} L={levels}")
    for c, used in LC.launches(LC.far(h, w, r), P):
        got = _volume(vols, dims, c, r, levels, extra)
        assert not got[:used].any()
        _same_bits(got, R.lookup64(planes, c, r)[0], "far")
    for variant in (0, 1):
        c, idx = LC.outlier(h, w, r, variant)
        got = _volume(vols, dims, c, r, levels, extra)
        assert not got[idx].any() and got.shape == (P, n)
        _same_bits(got, R.lookup64(planes, c, r)[0], f"outlier{variant}")


@pytest.mark.parametrize("bf16,r", [(False, 4), (False, 3), (True, 4), (True, 3)])
@pytest.mark.parametrize("h,w", LC.MAPS)
def test_volume_lookup_nonfinite_pixels_touch_only_their_own_row(h, w, bf16, r):
    """One pixel per block holds NaN, +Inf or -Inf (the CPU test shows that no address leaves its level): its row is
    unspecified, every other row is bit-equal to the run in which that pixel holds 3e9, and to lookup64."""
    vols, dims = _tiled(h, w, bf16)
    for variant in (0, 1):
        c, idx = LC.nonfinite(h, w, variant)
        s, _ = LC.nonfinite(h, w, variant, standin=True)
        got, ref = _volume(vols, dims, c, r), _volume(vols, dims, s, r)
        keep = np.ones(h * w, bool)
        keep[idx] = False
        _same_bits(got[keep], ref[keep], "nonfinite vs 3e9")
        _same_bits(ref, R.lookup64(LC.volume_planes(h, w), s, r)[0], "3e9")


def test_volume_lookup_rejects_bad_arguments():
    h, w, r = 9, 11, 4
    vols, dims = _tiled(h, w, False)
    cg = torch.from_numpy(LC.smooth(h, w)).cuda()
    g = Guarded(h * w, _nout(4, r), _nout(4, r), FILLS[0])
    lib = _lib.load()

    def params(**kw):
        p = ops.make_lookup_params(vols, dims, cg, g.view, r)
        for k, v in kw.items():
            if k in ("vol", "plane"):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p
    assert lib.woft_corr_lookup(C.byref(params()), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    g.buf.fill_(FILLS[0])
    small = ops.tiled_dims(*dims[1])[2] - 1
    for bad in (dict(levels=0), dict(levels=5), dict(radius=2), dict(ldo=_nout(4, r) - 1), dict(plane=(1, small)),
                dict(vol=(0, None)), dict(vol=(3, None)), dict(coords=None), dict(out=None), dict(n_pix=0)):
        assert lib.woft_corr_lookup(C.byref(params(**bad)), _lib.stream_ptr()) == EINVAL, bad
    torch.cuda.synchronize()
    assert bool((g.buf == FILLS[0]).all())


# ---- the volume-free lookup ------------------------------------------------------------------------------------------------------
def _operand(a, terms):
    """Feature rows (n, k) float32 -> the operand format of `terms`: 0 the fp32 rows, 1 one bf16 plane, 3 split-bf16 lines."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    if terms == 0:
        return t
    if terms == 1:
        o = torch.zeros(t.shape, dtype=torch.bfloat16, device="cuda")
        ops.split_bf16(t, o, None)
        return o
    o = torch.zeros(t.shape[0], 2 * t.shape[1], dtype=torch.bfloat16, device="cuda")
    ops.split_bf16_lines(t, o)
    return o


def _otf_params(f1s, f2s, dims, h, w, k, cg, out_view, r, terms, levels):
    return ops.make_lookup_otf_params(f1s, f2s[:levels], dims[:levels], h, w, k, cg, out_view, r, terms)


def _otf(f1s, f2s, dims, h, w, k, coords, r, terms, levels=4, extra=28):
    """woft_corr_lookup_otf into guarded outputs (guard columns beyond the channels) under both pre-fills."""
    cg = torch.from_numpy(np.ascontiguousarray(coords, np.float32)).cuda()
    outs = []
    for fill in FILLS:
        g = Guarded(h * w, _nout(levels, r), _nout(levels, r) + extra, fill)
        ops.run_lookup_otf(_otf_params(f1s, f2s, dims, h, w, k, cg, g.view, r, terms, levels))
        torch.cuda.synchronize()
        outs.append(g.numpy())
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "the two pre-fills disagree: an element was not written"
    return outs[0]


@pytest.mark.parametrize("terms", [0, 1, 3])
@pytest.mark.parametrize("h,w", LC.MAPS)
def test_otf_lookup_exact_features_against_fp64(h, w, terms):
    """Integer features (every product and sum exact in every operand format), k = 256 (alpha = 1/16), `exact` coordinates:
    bit-equal to lookup64 of the float64 correlation planes alpha f1 f2_l^T -- an independent reference, every level's f2 an
    independent map.  levels 4 and 2, ldo with and without guard columns; `far` gives exact zeros."""
    r, k, P = 4, 256, h * w
    f1, f2 = LC.exact_features(h, w, k)
    dims, corr = LC.level_dims(h, w), LC.corr_planes64(f1, f2, h, w, k)
    f1s, f2s = _operand(f1, terms), [_operand(b, terms) for b in f2]
    for levels, extra in ((4, 28), (2, 0)):
        for kk, (c, used) in enumerate(LC.launches(LC.exact(h, w, r), P)):
            want, _ = R.lookup64(corr[:levels], c, r)
            _same_bits(_otf(f1s, f2s, dims, h, w, k, c, r, terms, levels, extra), want, f"otf exact[{kk}] L={levels}")
    for c, used in LC.launches(LC.far(h, w, r), P):
        got = _otf(f1s, f2s, dims, h, w, k, c, r, terms)
        assert not got[:used].any()
        _same_bits(got, R.lookup64(corr, c, r)[0], "otf far")


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("h,w", LC.MAPS)
def test_otf_lookup_cross_terms_against_fp64(h, w, variant):
    """terms = 3 with a non-zero low plane in one operand (and a zero one in the other): the cross products a_lo b_hi / a_hi
    b_lo carry the low 8 bits, every sum is exact, coordinates with fractions 0 and 1/2 at every level: bit-equal to fp64."""
    r, k, P = 4, 256, h * w
    f1, f2 = LC.cross_features(h, w, variant, k)
    dims, corr = LC.level_dims(h, w), LC.corr_planes64(f1, f2, h, w, k)
    f1s, f2s = _operand(f1, 3), [_operand(b, 3) for b in f2]
    lo = (f1s if variant == 1 else f2s[0]).view(-1, 2, 32)[:, 1]
    assert bool((lo.float() != 0).any())                                    # the low plane really is in play
    for kk, (c, used) in enumerate(LC.launches(LC.half(h, w, r), P)):
        _same_bits(_otf(f1s, f2s, dims, h, w, k, c, r, 3), R.lookup64(corr, c, r)[0], f"cross{variant}[{kk}]")


@functools.lru_cache(maxsize=None)
def _random_pyramid(h, w, k):
    """Random features of k channels in the shipped arithmetic (split bf16): the volume the correlation GEMM builds (tiled, and
    read back as float64 planes) and the split operands of the volume-free kernel, from the same pooled maps."""
    g = torch.Generator().manual_seed(1000 * h + w)
    f1, f2 = torch.rand(1, k, h, w, generator=g) * 2 - 1, torch.rand(1, k, h, w, generator=g) * 2 - 1
    vols, dims = _build_pyramid_gpu(ops, f1, f2, "bf16x3", presplit=True)
    assert dims == LC.level_dims(h, w)
    a1, cur = ops.act_from_nchw(f1), ops.act_from_nchw(f2)

    def split(t):
        o = torch.zeros(t.shape[0], 2 * k, dtype=torch.bfloat16, device="cuda")
        ops.split_bf16_lines(t.contiguous(), o)
        return o
    f2s = []
    for l in range(4):
        f2s.append(split(cur.t))
        if l < 3:
            nxt = ops.new_act(1, cur.h // 2, cur.w // 2, k)
            ops.avgpool2(cur, nxt)
            cur = nxt
    torch.cuda.synchronize()
    planes = [ops.untile_planes(v, a, b).double().cpu().numpy() for v, (a, b) in zip(vols, dims)]
    return vols, dims, planes, split(a1.t), f2s


def _both(h, w, k, r, c, levels=4):
    """(volume-free output, volume output) for one coordinate field on the random pyramid."""
    vols, dims, planes, f1s, f2s = _random_pyramid(h, w, k)
    return _otf(f1s, f2s, dims, h, w, k, c, r, 3, levels), _volume(vols, dims, c, r, levels, 28)


@pytest.mark.parametrize("k,r", [(256, 4), (128, 3)])
@pytest.mark.parametrize("h,w", LC.MAPS)
def test_otf_lookup_random_features_against_volume_and_fp64(h, w, k, r):
    """Random features: the volume-free output is bit-equal to woft_corr_lookup in the volume the correlation GEMM builds from
    the same operands, and within LOOKUP_BAND M of lookup64 of that volume read back from the device -- on `band`, `far`, both
    `outlier` fields, `interior` right after an `outlier` launch (a box that is not cleared after one that was) and
    `nonfinite`; levels 4 and 2."""
    P = h * w
    planes = _random_pyramid(h, w, k)[2]
    for levels in (4, 2):
        for kk, (c, used) in enumerate(LC.launches(LC.band(h, w, r), P)):
            got, vol = _both(h, w, k, r, c, levels)
            _same_bits(got, vol, f"otf vs volume, band[{kk}] L={levels}")
            want, m = R.lookup64(planes[:levels], c, r)
            _in_band(got, want, m, f"otf band[{kk}] {h}x{w} k={k} r={r} L={levels}")
    for c, used in LC.launches(LC.far(h, w, r), P):
        got, vol = _both(h, w, k, r, c)
        _same_bits(got, vol, "otf vs volume, far")
        assert not got[:used].any()
    for variant in (0, 1):
        c, idx = LC.outlier(h, w, r, variant)
        got, vol = _both(h, w, k, r, c)
        _same_bits(got, vol, f"otf vs volume, outlier{variant}")
        want, m = R.lookup64(planes, c, r)
        _in_band(got, want, m, f"otf outlier{variant} {h}x{w} k={k}")
        assert not got[idx].any()
        if (h, w) == LC.INTERIOR_MAP:
            ci = LC.interior(r)
            vols, dims, _, f1s, f2s = _random_pyramid(h, w, k)
            vol = _volume(vols, dims, ci, r, 4, 28)
            _otf(f1s, f2s, dims, h, w, k, c, r, 3)                          # the outlier field again, and right after it ...
            got = _otf(f1s, f2s, dims, h, w, k, ci, r, 3)
            _same_bits(got, vol, "otf vs volume, interior after outlier")
            want, m = R.lookup64(planes, ci, r)
            _in_band(got, want, m, f"otf interior after outlier{variant} k={k}")
        c, idx = LC.nonfinite(h, w, variant)
        s, _ = LC.nonfinite(h, w, variant, standin=True)
        (got, _), (ref, vol) = _both(h, w, k, r, c), _both(h, w, k, r, s)
        keep = np.ones(P, bool)
        keep[idx] = False
        _same_bits(got[keep], ref[keep], "otf nonfinite vs 3e9")
        _same_bits(ref, vol, "otf vs volume, 3e9")
        assert not ref[idx].any()


def test_otf_lookup_need_map_on_outlier_field():
    """With a `need` map the blocks without a wanted pixel are left untouched (pre-fill intact), the others are bit-equal to
    the run without the map -- on the `outlier` field, whose every block has a clipped box."""
    h, w, k, r = 17, 25, 256, 4
    vols, dims, planes, f1s, f2s = _random_pyramid(h, w, k)
    c, _ = LC.outlier(h, w, r, 0)
    full = _otf(f1s, f2s, dims, h, w, k, c, r, 3)
    need = torch.zeros(h, w, dtype=torch.int32, device="cuda")
    need[16, 24], need[9, 3] = 1, 7                                         # blocks (2, 3) and (1, 0)
    wanted = np.zeros((h, w), bool)
    wanted[16:, 24:], wanted[8:16, 0:8] = True, True
    wanted = wanted.reshape(-1)
    cg = torch.from_numpy(c).cuda()
    for fill in FILLS:
        g = Guarded(h * w, _nout(4, r), _nout(4, r) + 28, fill)
        p = _otf_params(f1s, f2s, dims, h, w, k, cg, g.view, r, 3, 4)
        p.need = need.data_ptr()
        ops.run_lookup_otf(p)
        torch.cuda.synchronize()
        got = g.numpy()
        _same_bits(got[wanted], full[wanted], "wanted blocks")
        assert (got[~wanted] == np.float32(fill)).all()


def test_otf_lookup_rejects_bad_arguments():
    h, w, k, r = 9, 11, 256, 4
    vols, dims, planes, f1s, f2s = _random_pyramid(h, w, k)
    cg = torch.from_numpy(LC.smooth(h, w)).cuda()
    g = Guarded(h * w, _nout(4, r), _nout(4, r), FILLS[0])
    part = torch.zeros(h * w, 20, device="cuda")
    delta, need = torch.zeros(h * w, 4, device="cuda"), torch.ones(h, w, dtype=torch.int32, device="cuda")
    lib = _lib.load()

    def params(**kw):
        p = _otf_params(f1s, f2s, dims, h, w, k, cg, g.view, r, 3, 4)
        for name, v in kw.items():
            if name in ("h", "w", "f2"):
                getattr(p, name)[v[0]] = v[1]
            else:
                setattr(p, name, v)
        return p
    fh = dict(fh_part=part.data_ptr(), fh_delta=delta.data_ptr(), fh_planes=1, fh_ld=20, fh_ld_delta=4)
    for bad in (dict(terms=2), dict(k=96), dict(h=(2, 0)), dict(ldo=_nout(4, r) - 1), dict(fh, need=need.data_ptr()),
                dict(fh, fh_delta=None), dict(fh, fh_ld=18), dict(fh, fh_ld=22), dict(fh, fh_planes=0), dict(fh, fh_ld_delta=1),
                dict(levels=0), dict(levels=5), dict(radius=2), dict(f2=(1, None)), dict(coords=None)):
        assert lib.woft_corr_lookup_otf(C.byref(params(**bad)), _lib.stream_ptr()) == EINVAL, bad
    torch.cuda.synchronize()
    assert bool((g.buf == FILLS[0]).all()) and not bool(delta.any())


# ---- the folded flow-head gather ------------------------------------------------------------------------------------------------
def _gather_two_ways(h, w, part, n_planes, bias, start, ld_delta, cat_ld, cat_col, fill, k=256, r=4, with_cat=True):
    """Launch A: woft_flow_head_gather, then the plain volume-free lookup.  Launch B: one lookup launch with the fh_* fields, on
    copies of the same buffers.  -> two dicts of numpy arrays (coords, delta, flow4, flow_cat, out), guards asserted."""
    vols, dims, planes, f1s, f2s = _random_pyramid(h, w, k)
    P = h * w
    res = []
    for folded in (False, True):
        coords = Guarded(P, 2, 2, fill).put(start)
        delta, flow4 = Guarded(P, 2, ld_delta, fill), Guarded(P, 4, 4, fill)
        cat = Guarded(P, 2, cat_ld, fill, col0=cat_col)
        out = Guarded(P, _nout(4, r), _nout(4, r) + 28, fill)
        p = _otf_params(f1s, f2s, dims, h, w, k, coords.view, out.view, r, 3, 4)
        if folded:
            p.fh_part, p.fh_bias, p.fh_delta = part.data_ptr(), None if bias is None else bias.data_ptr(), delta.ptr()
            p.fh_flow4, p.fh_flow_cat = flow4.ptr(), cat.ptr() if with_cat else None
            p.fh_planes, p.fh_ld, p.fh_ld_delta, p.fh_ld_cat = n_planes, part.shape[1], ld_delta, cat_ld
        else:
            ops.flow_head_gather(part, n_planes, h, w, bias, types.SimpleNamespace(t=delta.view, cs=ld_delta), coords.view,
                                 flow4.view, cat.view if with_cat else None, cat_ld)
        ops.run_lookup_otf(p)
        torch.cuda.synchronize()
        res.append(dict(coords=coords.numpy(), delta=delta.numpy(), flow4=flow4.numpy(),
                        flow_cat=cat.numpy() if with_cat else cat.numpy(0), out=out.numpy()))
    return res


def _check_gather(h, w, part, n_planes, bias, start, a, b, exact=False):
    for name in a:
        _same_bits(a[name], b[name], f"folded gather: {name}")
    want, mag = R.flow_head_gather64(part.cpu().numpy(), n_planes, h, w, None if bias is None else bias.cpu().numpy())
    err = np.abs(b["delta"].astype(np.float64) - want)
    assert (err <= R.gather_band(n_planes, mag)).all(), float((err / np.maximum(mag, 1e-300)).max() / R.U32)
    if exact:
        assert np.array_equal(b["delta"].astype(np.float64), want)
    start = np.asarray(start, np.float32)
    assert np.array_equal(_bits(b["coords"]), _bits(start + b["delta"]))    # float32(start + delta), exactly
    ys, xs = np.mgrid[0:h, 0:w]
    grid = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.float32)
    assert np.array_equal(_bits(b["flow4"][:, :2]), _bits(b["coords"] - grid)) and not b["flow4"][:, 2:].any()
    if b["flow_cat"].size:
        assert np.array_equal(_bits(b["flow_cat"]), _bits(b["flow4"][:, :2]))


@pytest.mark.parametrize("fh_ld", [20, 24])
@pytest.mark.parametrize("n_planes", [1, 2, 4])
@pytest.mark.parametrize("h,w", LC.MAPS)
def test_folded_gather_equals_two_launches_and_fp64(h, w, n_planes, fh_ld):
    """The lookup launch that also performs the previous iteration's 3x3 gather, coords1 += delta and the flow operands, against
    woft_flow_head_gather + the plain lookup (bit for bit: coords, delta, flow4, flow_cat and the lookup output) and against
    flow_head_gather64 (the fixed-order summation bound); start coordinates from the `band` list; fh_ld_delta 4 and wider, the
    flow_cat pair inside a wider guarded row, once without a bias, once without flow_cat."""
    P = h * w
    g = torch.Generator().manual_seed(100 * h + 10 * n_planes + fh_ld)
    part = torch.randn(n_planes * P, fh_ld, generator=g).cuda()
    bias = torch.randn(2, generator=g).cuda()
    starts = [c for c, _ in LC.launches(LC.band(h, w, 4), P)]
    settings = [(bias, 4, 12, 6, True), (None, 6, 2, 0, True), (bias, 2, 5, 3, False)]
    for n, (bs, ld_delta, cat_ld, cat_col, with_cat) in enumerate(settings):
        start = starts[n % len(starts)]
        a, b = _gather_two_ways(h, w, part, n_planes, bs, start, ld_delta, cat_ld, cat_col, FILLS[n % 2], with_cat=with_cat)
        _check_gather(h, w, part, n_planes, bs, start, a, b)


@pytest.mark.parametrize("h,w", LC.MAPS)
def test_folded_gather_border_taps_are_zero_exactly(h, w):
    """An integer-valued `part` (every sum exact in any order): delta of both paths is the float64 sum bit for bit, so a tap
    outside the grid that was not zeroed, at any border pixel, shows as a wrong integer."""
    P, n_planes = h * w, 2
    rs = np.random.RandomState([h, w, 9])
    part = torch.from_numpy(rs.randint(-64, 65, (n_planes * P, 20)).astype(np.float32)).cuda()
    bias = torch.tensor([3.0, -5.0], device="cuda")
    start = LC.smooth(h, w)
    for fill in FILLS:
        a, b = _gather_two_ways(h, w, part, n_planes, bias, start, 4, 4, 2, fill)
        _check_gather(h, w, part, n_planes, bias, start, a, b, exact=True)
        assert np.array_equal(a["delta"].astype(np.float64), R.flow_head_gather64(part.cpu().numpy(), n_planes, h, w,
                                                                                  bias.cpu().numpy())[0])


# ---- convex upsampling ----------------------------------------------------------------------------------------------------------
def _convex(coords, wlow, mask, hf, wf, crop, h, w, which, fill, sigmoid=False):
    """woft_convex_upsample with the outputs named in `which` (of flow_up, dst, wout) into guarded buffers."""
    lib = _lib.load()
    bufs = {"flow_up": Guarded(2, h * w, h * w, fill), "dst": Guarded(2, h * w, h * w, fill), "wout": Guarded(1, h * w, h * w, fill)}
    rc = lib.woft_convex_upsample(coords.data_ptr(), None if wlow is None else wlow.data_ptr(), mask.data_ptr(), mask.shape[1],
                                  hf, wf, crop[0], crop[1], h, w, *[bufs[n].ptr() if n in which else None for n in bufs],
                                  int(sigmoid), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    got = {n: b.numpy() for n, b in bufs.items()}
    for n in bufs:
        if n not in which or (n == "wout" and wlow is None):
            assert (got[n] == np.float32(fill)).all(), f"{n} written without being asked for"
    return got


@pytest.mark.parametrize("ld_mask", [576, 640])
@pytest.mark.parametrize("hf,wf", LC.CONVEX_SHAPES)
def test_convex_upsample_against_fp64(hf, wf, ld_mask):
    """Grids one cell high or wide (most of the 3x3 support outside the grid), a cell whose logits are +-80 (the softmax collapses
    onto one tap, nothing overflows), mask rows wider than 576 (the padding holds NaN: reading it would show), wlow null, each
    output alone, the full frame and the maximal crop (crop_top + h = 8 hf): within CONVEX_BAND max |8 v_k| of the float64
    softmax and sum; dst is float32(x) + flow_up exactly; all outputs agree between the call forms and the two pre-fills."""
    coords, wlow, mask = LC.convex_case(hf, wf, ld_mask)
    mask[:, 576:] = np.nan
    v, _ = LC.convex_values(coords, wlow, hf, wf)
    want, m = R.convex_upsample64(v, mask, hf, wf)
    cd, wd, md = torch.from_numpy(coords).cuda(), torch.from_numpy(wlow).cuda(), torch.from_numpy(mask).cuda()
    H, W = 8 * hf, 8 * wf
    for top, left, h, w in ((0, 0, H, W), (3, 2, H - 3, W - 2), (H - 1, W - 1, 1, 1)):
        assert top + h == H and left + w == W
        sl = (slice(top, top + h), slice(left, left + w))
        all3 = _convex(cd, wd, md, hf, wf, (top, left), h, w, ("flow_up", "dst", "wout"), FILLS[0])
        for n in ("flow_up", "dst", "wout"):
            alone = _convex(cd, wd, md, hf, wf, (top, left), h, w, (n,), FILLS[1])
            _same_bits(alone[n], all3[n], f"{n} alone")
        none = _convex(cd, None, md, hf, wf, (top, left), h, w, ("flow_up", "dst", "wout"), FILLS[1])     # wlow null: no wout
        _same_bits(none["flow_up"], all3["flow_up"], "flow_up without wlow")
        _same_bits(none["dst"], all3["dst"], "dst without wlow")
        fu = all3["flow_up"].reshape(2, h, w)
        assert np.isfinite(fu).all() and np.isfinite(all3["wout"]).all()
        got3 = np.concatenate([fu.astype(np.float64), 8.0 * all3["wout"].reshape(1, h, w)])   # wout = (sum s 8 wlow) / 8, exactly
        err, mm = np.abs(got3 - want[(slice(None),) + sl]), m[(slice(None),) + sl]
        print(f"CONVEX {hf}x{wf} ld_mask {ld_mask} crop ({top}, {left}): largest error "
              f"{float((err[mm > 0] / mm[mm > 0]).max() / R.U32):.2f} units of 2^-24 max |8 v|")
        assert (err <= R.CONVEX_BAND * mm).all()
        ys, xs = np.mgrid[0:h, 0:w]
        _same_bits(all3["dst"].reshape(2, h, w), np.stack([xs.astype(np.float32) + fu[0], ys.astype(np.float32) + fu[1]]), "dst")
        # 1 / (1 + expf(-v)): an ulp or two in expf weighs s (1 - s) <= 1/4, the sum and the division half an ulp of a number <= 1 each
        sg = _convex(cd, wd, md, hf, wf, (top, left), h, w, ("wout",), FILLS[0], sigmoid=True)["wout"].astype(np.float64)
        assert np.abs(sg - 1 / (1 + np.exp(-all3["wout"].astype(np.float64)))).max() <= 4 * R.U32


@pytest.mark.parametrize("hf,wf", LC.CONVEX_SHAPES)
def test_convex_weights_at_corners_and_counts(hf, wf):
    """woft_convex_weights_at stays bit-equal to the full kernel at the four image corners and the crop's corners; count 0
    writes nothing; a count above n_max is clamped to n_max."""
    coords, wlow, mask = LC.convex_case(hf, wf, 640)
    mask[:, 576:] = np.nan
    cd, wd, md = torch.from_numpy(coords).cuda(), torch.from_numpy(wlow).cuda(), torch.from_numpy(mask).cuda()
    H, W = 8 * hf, 8 * wf
    for top, left, h, w in ((0, 0, H, W), (3, 2, H - 3, W - 2)):
        full = _convex(cd, wd, md, hf, wf, (top, left), h, w, ("wout",), FILLS[0])["wout"].reshape(h, w)
        pts = np.array([(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2), (w - 1, h // 3)], np.float32)
        n_max = len(pts)
        pd = torch.from_numpy(pts).cuda()
        for count, n_written in ((n_max, n_max), (0, 0), (4, 4), (n_max + 5, n_max)):
            for fill in FILLS:
                g = Guarded(1, n_max, n_max, fill)
                cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
                rc = _lib.load().woft_convex_weights_at(pd.data_ptr(), cnt.data_ptr(), n_max, wd.data_ptr(), md.data_ptr(), 640,
                                                        hf, wf, top, left, 0, g.ptr(), _lib.stream_ptr())
                assert rc == 0
                torch.cuda.synchronize()
                got = g.numpy()[0]
                _same_bits(got[:n_written], full[pts[:n_written, 1].astype(int), pts[:n_written, 0].astype(int)], "weights_at")
                assert (got[n_written:] == np.float32(fill)).all()
