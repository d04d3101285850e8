"""The references and inputs of test_lookup_edges_gpu, checked without a GPU and without the library: the coordinate lists cover
the edges and tile phases they claim, the exact data is exactly representable where the GPU test demands bit equality, a host
restatement of both lookup kernels' index arithmetic (lookup_host.py) keeps every address of every list inside its level, the
fp64 references agree with the oracle's direct formula, and fp32 restatements of the kernels' arithmetic stay inside the bands
of fp64_refs (LOOKUP_BAND, gather_band, CONVEX_BAND) with zero violations -- and are bit-equal where the data is exact.  The
references raise no floating-point warning on finite input (every test here runs with warnings turned into errors)."""
import numpy as np
import pytest
import torch

from oracle import raft_ref
import fp64_refs as R
import lookup_cases as LC
import lookup_host as LH


@pytest.fixture(autouse=True)
def _raise_on_fp_warnings():
    with np.errstate(all="raise"):
        yield


def _lists(h, w, r):
    """Every coordinate set that goes to a GPU on this map, as launches of P pairs: [(name, coords (P, 2))]."""
    P = h * w
    out = []
    for name in ("exact", "band", "far"):
        out += [(f"{name}[{k}]", c) for k, (c, _) in enumerate(LC.launches(getattr(LC, name)(h, w, r), P))]
    out += [(f"half[{k}]", c) for k, (c, _) in enumerate(LC.launches(LC.half(h, w, r), P))]
    for v in (0, 1):
        out += [(f"outlier{v}", LC.outlier(h, w, r, v)[0]), (f"nonfinite{v}", LC.nonfinite(h, w, v)[0]),
                (f"standin{v}", LC.nonfinite(h, w, v, standin=True)[0])]
    if (h, w) == LC.INTERIOR_MAP:
        out.append(("interior", LC.interior(r)))
    return out


# ---- coverage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", LC.RADII)
@pytest.mark.parametrize("h,w", LC.MAPS)
def test_exact_list_covers_edges_corners_and_tile_phases(h, w, r):
    pts = LC.exact(h, w, r).astype(np.float64)
    assert np.array_equal(pts * 4, np.rint(pts * 4))                        # multiples of 1/4
    for l, (hl, wl) in enumerate(LC.level_dims(h, w)):
        s = pts / 2.0 ** l
        fl, fr = np.floor(s), s - np.floor(s)
        assert np.array_equal(fr * 32, np.rint(fr * 32))                    # fractions: multiples of 1/32
        for axis, n in ((0, wl), (1, hl)):
            for f in LC.edge_floors(n, r):
                at = fl[:, axis] == f
                assert (at & (fr[:, axis] == 0)).any() and (at & (fr[:, axis] != 0)).any(), (l, axis, f)
        ex, ey = np.isin(fl[:, 0], LC.edge_floors(wl, r)), np.isin(fl[:, 1], LC.edge_floors(hl, r))
        assert (ex & ey).sum() >= 24                                        # corners: both axes at an edge
        wx0, wy0 = fl[:, 0].astype(np.int64) - r, fl[:, 1].astype(np.int64) - r
        for neg in (True, False):
            sel = (wx0 < 0) & (wy0 < 0) if neg else (wx0 >= 0) & (wy0 >= 0)
            assert len(set(zip((wx0[sel] % 4).tolist(), (wy0[sel] % 4).tolist()))) == 16, (l, neg)


@pytest.mark.parametrize("r", LC.RADII)
@pytest.mark.parametrize("h,w", LC.MAPS)
def test_band_far_outlier_and_nonfinite_lists(h, w, r):
    b = LC.band(h, w, r)
    assert b.dtype == np.float32 and len(b) >= 300
    for l in (0, 3):                                                        # one float below and above every integer edge
        for axis, n in ((0, max(w >> l, 1)), (1, max(h >> l, 1))):
            for f in LC.edge_floors(n, r):
                e = np.float32(2.0 ** l * f)
                with np.errstate(under="ignore"):                           # (the neighbours of 0 are subnormal)
                    lo, hi = np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))
                assert lo < e < hi and (b[:, axis] == lo).any() and (b[:, axis] == hi).any()
    fv = LC.far_values(r).astype(np.float64)
    for v in (1e6 - 0.5, 1e6 + 0.5, 1.5e6, 3e9, float(np.float32(1e30))):
        assert (fv == v).any() and (fv == -v).any()
    for l in range(LC.LEVELS):                                              # the window origin lands on +-16384 + d
        for sgn in (1, -1):
            org = np.floor(fv[np.abs(fv) < 1e6] / 2.0 ** l) - r
            assert set(org.astype(np.int64).tolist()) >= {sgn * 16384 + d for d in (-1, 0, 1)}
    f = LC.far(h, w, r).astype(np.float64)
    inx, iny = (f[:, 0] >= 0) & (f[:, 0] < w), (f[:, 1] >= 0) & (f[:, 1] < h)
    assert (inx & ~iny).sum() == len(fv) and (~inx & iny).sum() == len(fv) and (~inx & ~iny).sum() == len(fv)
    planes = LC.volume_planes(h, w)
    for c, n in LC.launches(f, h * w):                                      # every far row is all zeros, at every level
        v, m = R.lookup64(planes, c, r)
        assert not v[:n].any() and not m[:n].any()
    for variant in (0, 1):
        for c, idx in (LC.outlier(h, w, r, variant), LC.nonfinite(h, w, variant)):
            assert c.shape == (h * w, 2) and len(idx) == len(LC.blocks(h, w)) == len(set(idx.tolist()))
            plain = np.ones(h * w, bool)
            plain[idx] = False
            assert np.array_equal(c[plain], LC.smooth(h, w)[plain])         # exactly one pixel per block differs
            assert sorted({(i // w // 8, i % w // 8) for i in idx.tolist()}) == LC.blocks(h, w)
        c, idx = LC.nonfinite(h, w, variant)
        assert not np.isfinite(c[idx, variant]).any() and np.isfinite(np.delete(c, idx, 0)).all()
        s, _ = LC.nonfinite(h, w, variant, standin=True)
        assert (np.abs(s[idx, variant]) == 3e9).all() and np.array_equal(np.delete(s, idx, 0), np.delete(c, idx, 0))
        v, _ = R.lookup64(planes, c, r)                                     # a non-finite pixel reads nothing, without a warning
        assert not v[idx].any() and np.isfinite(v).all()
    hp = LC.half(h, w, r).astype(np.float64)
    for l in range(LC.LEVELS):
        fr = hp / 2.0 ** l - np.floor(hp / 2.0 ** l)
        assert np.isin(fr, (0.0, 0.5)).all()


# ---- representability -----------------------------------------------------------------------------------------------------------
def _is_f32(v):
    return np.array_equal(np.asarray(v, np.float64), np.asarray(v, np.float64).astype(np.float32).astype(np.float64))


def _bf16_round_trip(a):
    t = torch.from_numpy(np.array(a, np.float32))
    return torch.equal(t.to(torch.bfloat16).float(), t)


@pytest.mark.parametrize("r", LC.RADII)
@pytest.mark.parametrize("h,w", LC.MAPS)
def test_exact_data_is_exactly_representable(h, w, r):
    """Where the GPU test demands bit equality the float64 result must be a float32 number, and the fp32 restatement of the
    kernels' lerps must produce exactly it: volume planes (also exact in bf16) and correlations of the exact features under
    the `exact` list; the cross-term features under the `half` list."""
    P = h * w
    planes = LC.volume_planes(h, w)
    assert all(_bf16_round_trip(p) and np.abs(p).max() <= 256 for p in planes)
    f1, f2 = LC.exact_features(h, w)
    assert _bf16_round_trip(f1) and all(_bf16_round_trip(b) for b in f2)
    corr = LC.corr_planes64(f1, f2, h, w)
    assert all(_is_f32(c) and np.array_equal(c * 16, np.rint(c * 16)) and np.abs(c).max() < 64 for c in corr)
    for c, _ in LC.launches(LC.exact(h, w, r), P):
        assert _is_f32(c)
        for pl in (planes, corr):
            v, _ = R.lookup64(pl, c, r)
            assert _is_f32(v)
            assert np.array_equal(LH.lookup32(pl, c, r).astype(np.float64), v)
    for variant in (0, 1):
        a, b = LC.cross_features(h, w, variant)
        fine, coarse = ([a], b) if variant == 1 else (b, [a])
        assert all(_bf16_round_trip(x) for x in coarse)                     # a zero low plane
        for x in fine:                                                      # hi + lo is the value, in two bf16 numbers
            t = torch.from_numpy(x)
            hi = t.to(torch.bfloat16).float()
            lo = (t - hi).to(torch.bfloat16).float()
            assert torch.equal(hi + lo, t) and bool((lo != 0).any())
        corr = LC.corr_planes64(a, b, h, w)
        # every product is a multiple of 2^-8 and every partial sum stays below 2^10: an fp32 accumulator holds it in any order
        assert all(_is_f32(c) and np.array_equal(c * 4096, np.rint(c * 4096)) for c in corr)
        assert 256 * 2 * 2 <= 2 ** 10
        for c, _ in LC.launches(LC.half(h, w, r), P):
            v, _ = R.lookup64(corr, c, r)
            assert _is_f32(v) and np.array_equal(LH.lookup32(corr, c, r).astype(np.float64), v)


# ---- the index arithmetic of both kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", LC.RADII)
@pytest.mark.parametrize("h,w", LC.MAPS)
def test_every_address_of_every_list_stays_inside_its_level(h, w, r):
    """Before any of these lists goes to a GPU: the tiles the volume kernel loads, the rows the volume-free kernel streams and
    the window cells its values land in lie inside their arrays for every coordinate, non-finite ones included."""
    dims = LC.level_dims(h, w)
    clipped = {}
    for name, c in _lists(h, w, r):
        assert c.shape == (h * w, 2) and c.dtype == np.float32
        assert LH.check_volume_indices(c, dims, r) > 0 or name.startswith("far")
        for levels in (4, 2):
            clipped[name] = LH.check_otf_indices(c, h, w, dims[:levels], r)
    if (h, w) == LC.INTERIOR_MAP:                                           # the box that is not cleared, after one that was
        key = LC.INTERIOR_BLOCK + (0,)
        assert not clipped["interior"][key] and clipped["outlier0"][key] and clipped["outlier1"][key]
        assert clipped["interior"][(0, 0, 0)]


# ---- the references -------------------------------------------------------------------------------------------------------------
def test_lookup64_is_the_direct_formula_of_the_oracle():
    rs = np.random.RandomState(5)
    h, w = 7, 9
    P = h * w
    planes = [rs.standard_normal((P, a, b)) for a, b in ((13, 10), (6, 5), (3, 2), (1, 1))]
    coords = np.stack([rs.uniform(-8, 17, P), rs.uniform(-8, 20, P)], 1)
    ct = torch.from_numpy(coords.T.reshape(1, 2, h, w).copy())
    for r in LC.RADII:
        want = raft_ref.lookup_direct([torch.from_numpy(p)[:, None] for p in planes], ct, r)
        assert want.dtype == torch.float64
        got, m = R.lookup64(planes, coords, r)
        assert np.abs(got - want[0].permute(1, 2, 0).reshape(P, -1).numpy()).max() <= 1e-12
        assert (np.abs(got) <= m * (1 + 1e-12)).all()                       # a convex combination of its taps


ORACLE_DISTANCE = 2.0 ** -18     # of the largest |value| of the pyramid: twice the measured 1.2e-6, rounded up to a power of two
#                                  (profiles/README.md)


def test_grid_sample_oracle_is_farther_from_fp64_than_the_band():
    """Why the new tests do not use raft_ref.corr_lookup: its normalise / un-normalise round trip costs more than the whole
    band of the kernels' arithmetic.  On the `band` list of the (17, 25) map (the only one whose levels are all wider than one
    pixel: the oracle divides by W - 1) it lies within ORACLE_DISTANCE of lookup64, and beyond LOOKUP_BAND somewhere."""
    h, w, r = 17, 25, 4
    P = h * w
    rs = np.random.RandomState(6)
    planes = [rs.standard_normal((P, a, b)).astype(np.float32) for a, b in LC.level_dims(h, w)]
    top = max(float(np.abs(p).max()) for p in planes)
    worst, beyond = 0.0, 0
    for c, n in LC.launches(LC.band(h, w, r), P):
        ct = torch.from_numpy(c.T.reshape(1, 2, h, w).copy())
        with np.errstate(all="ignore"):
            got = raft_ref.corr_lookup([torch.from_numpy(p)[:, None] for p in planes], ct, r)[0].permute(1, 2, 0).reshape(P, -1)
        want, m = R.lookup64(planes, c, r)
        d = np.abs(got.numpy().astype(np.float64) - want)[:n]
        worst, beyond = max(worst, float(d.max())), beyond + int((d > R.LOOKUP_BAND * np.maximum(m[:n], 1e-30)).sum())
    print(f"LOOKUP oracle-to-fp64 distance on band(17, 25): {worst:.3e} = {worst / top:.3e} of the largest value {top:.2f}; "
          f"samples beyond LOOKUP_BAND * M: {beyond}")
    assert worst <= ORACLE_DISTANCE * top
    assert beyond > 0


def test_lerp_restatement_stays_inside_the_band():
    """LOOKUP_BAND is twice the largest error of the fp32 restatement, in units of 2^-24 M, rounded up to a power of two: on
    the `band` lists of all maps and on seeded random samples (more than a million) the restatement has zero violations and
    its largest error lies in (LOOKUP_BAND / 4, LOOKUP_BAND / 2] units -- the constant is neither too tight nor slack."""
    worst = 0.0
    cases = [(h, w, r, c) for h, w in LC.MAPS for r in LC.RADII for c, _ in LC.launches(LC.band(h, w, r), h * w)]
    rs = np.random.RandomState(7)
    h, w = 40, 50
    cases += [(h, w, 4, np.stack([rs.uniform(-8, w + 8, h * w), rs.uniform(-8, h + 8, h * w)], 1).astype(np.float32))
              for _ in range(2)]
    n = 0
    for h, w, r, c in cases:
        prs = np.random.RandomState([h, w, r])
        planes = [prs.standard_normal((h * w, a, b)).astype(np.float32) for a, b in LC.level_dims(h, w)]
        want, m = R.lookup64(planes, c, r)
        err = np.abs(LH.lookup32(planes, c, r).astype(np.float64) - want)
        assert (err <= R.LOOKUP_BAND * m).all(), (h, w, r, float((err / np.maximum(m, 1e-300)).max() / R.U32))
        worst, n = max(worst, float((err[m > 0] / m[m > 0]).max() / R.U32)), n + err.size
    print(f"LOOKUP lerp restatement: {n} samples, largest error {worst:.2f} units of 2^-24 M; LOOKUP_BAND = "
          f"{R.LOOKUP_BAND / R.U32:.0f} units")
    assert n > 1_000_000 and R.LOOKUP_BAND / 4 < worst * R.U32 <= R.LOOKUP_BAND / 2


@pytest.mark.parametrize("n_planes", [1, 2, 4])
@pytest.mark.parametrize("h,w", LC.MAPS)
def test_gather_restatement_against_fp64(h, w, n_planes):
    rs = np.random.RandomState([h, w, n_planes])
    part = rs.standard_normal((n_planes * h * w, 24)).astype(np.float32)
    bias = rs.standard_normal(2).astype(np.float32)
    for b in (bias, None):
        want, mag = R.flow_head_gather64(part, n_planes, h, w, b)
        got = LH.gather32(part, n_planes, h, w, b)
        assert (np.abs(got.astype(np.float64) - want) <= R.gather_band(n_planes, mag)).all()
        assert (np.abs(want) <= mag).all()
    # the border: a direct loop over the taps of the four corner pixels and one interior pixel
    want, _ = R.flow_head_gather64(part, n_planes, h, w, bias)
    pt = part.astype(np.float64).reshape(-1, 24)
    for y, x in {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)}:
        d = bias.astype(np.float64).copy()
        for ky in range(3):
            for kx in range(3):
                yy, xx = y + ky - 1, x + kx - 1
                if 0 <= yy < h and 0 <= xx < w:
                    for p in range(n_planes):
                        d += pt[p * h * w + yy * w + xx, (3 * ky + kx) * 2:(3 * ky + kx) * 2 + 2]
        assert np.abs(d - want[y * w + x]).max() <= 1e-12
    ipart = rs.randint(-64, 65, (n_planes * h * w, 20)).astype(np.float32)  # integers: exact in any order
    want, _ = R.flow_head_gather64(ipart, n_planes, h, w, np.array([3.0, -5.0]))
    assert np.array_equal(LH.gather32(ipart, n_planes, h, w, np.array([3.0, -5.0], np.float32)).astype(np.float64), want)


@pytest.mark.parametrize("hf,wf", LC.CONVEX_SHAPES)
def test_convex_restatement_stays_inside_the_band(hf, wf):
    coords, wlow, mask = LC.convex_case(hf, wf)
    v, v8 = LC.convex_values(coords, wlow, hf, wf)
    want, m = R.convex_upsample64(v, mask, hf, wf)
    got = LH.convex32(v8, mask, hf, wf).astype(np.float64)
    err = np.abs(got - want)
    worst = float((err[m > 0] / m[m > 0]).max() / R.U32)
    print(f"CONVEX restatement {hf}x{wf}: largest error {worst:.2f} units of 2^-24 max |8 v|; CONVEX_BAND = "
          f"{R.CONVEX_BAND / R.U32:.0f} units")
    assert (err <= R.CONVEX_BAND * m).all() and np.isfinite(got).all()
    assert (np.abs(want) <= m * (1 + 1e-12)).all()                          # a convex combination
    cell = (hf * wf) // 2                                                   # the collapsed cell: a tap at -80 beside one at +80
    s = np.exp(mask[cell, :576].astype(np.float64).reshape(9, 64) - 80.0)  # weighs e^-160: nothing in fp32
    assert (s / s.sum(0)).min() < 1e-60
