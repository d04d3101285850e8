"""The references and inputs of test_image_geometry_gpu, checked without a GPU: the fp32 oracle (oracle/tracker_ref.py) obeys the
classification rule against the fp64 references for every generic case, every excused share is within the cap, every exact
case's analytic inverse is what np.linalg.inv returns bit for bit, the integer-arithmetic expectations are what the fp64
references round to, and the references raise no floating-point warning outside their explicit guards."""
import numpy as np
import pytest

from oracle import tracker_ref
import fp64_refs as R
import geometry_cases as G


@pytest.fixture(autouse=True)
def _raise_on_fp_warnings():
    """Every reference call in this module runs with all floating-point warnings turned into errors."""
    with np.errstate(all="raise"):
        yield


@pytest.mark.parametrize("hname", list(G.GENERIC))
@pytest.mark.parametrize("c", G.CHANNELS)
@pytest.mark.parametrize("h,w", G.SIZES)
def test_oracle_obeys_the_rule_and_the_caps_hold(h, w, c, hname):
    img, Hm = G.image(h, w, c), G.GENERIC[hname]
    v, sx, sy = R.warp_linear64(img, Hm)
    assert v.dtype == np.float64 and v.shape == img.shape and np.isfinite(v).all()
    with np.errstate(all="ignore"):                    # the fp32 oracle casts huge coordinates: its own business, not the rule's
        got = tracker_ref.warp_linear_u8(img, Hm)
        got_valid = tracker_ref.warp_linear(np.ones((h, w)), Hm) > 0
        got_near = tracker_ref.warp_nearest(img.reshape(h, w, -1)[..., 0], Hm)     # (the oracle's takes one channel)
    bad, excused, used = R.classify_bytes(v, got)
    assert not bad.any(), (int(bad.sum()), v[bad][:5], got[bad][:5])
    assert G.share(excused) <= G.CAP and not (used & ~excused).any()
    valid, vex = R.warp_valid64(sx, sy, h, w), R.warp_valid_excused(sx, sy, h, w)
    assert G.share(vex) <= G.CAP and np.array_equal(got_valid[~vex], valid[~vex])
    near, _, _, inside = R.warp_nearest64(img, Hm)
    nex = R.warp_nearest_excused(sx, sy, h, w)
    assert G.share(nex) <= G.CAP and np.array_equal(got_near[~nex], near.reshape(h, w, -1)[..., 0][~nex])
    assert not (inside & ~valid & ~vex).any()          # a pixel that reads a source pixel has a tap with positive weight
    if (h, w) in G.THIN:
        assert not excused.any() and not vex.any() and not nex.any()
    if hname == "horizon-inv" and (h, w) in G.CROSSED:
        d = R.warp_source64(h, w, Hm)[2]
        assert (d > 0).any() and (d < 0).any()         # the horizon really crosses the frame
        assert (np.abs(sx[np.isfinite(sx)]) > 10 * w).any()                 # and leaves huge finite coordinates beside it


@pytest.mark.parametrize("c", G.CHANNELS)
@pytest.mark.parametrize("h,w", G.SIZES)
def test_exact_zero_denominator_and_far(h, w, c):
    img = G.case_image("dzero", h, w, c)
    Hm, Hinv, k = G.dzero(h, w)
    assert np.array_equal(np.linalg.inv(Hm), Hinv)                          # bit for bit (0.0 == -0.0 aside)
    v, sx, sy = R.warp_linear64(img, Hm)
    ys, xs = np.mgrid[0:h, 0:w]
    zero = xs + ys == k
    assert zero.any() and np.array_equal(R.warp_source64(h, w, Hm)[2] == 0, zero)
    assert np.isinf(sx[zero]).all() and np.isinf(sy[zero]).all() and not np.isnan(sx).any() and not np.isnan(sy).any()
    assert (v.reshape(h, w, -1)[zero] == 0).all() and not R.warp_valid64(sx, sy, h, w)[zero].any()
    near, _, _, inside = R.warp_nearest64(img, Hm)
    assert (near.reshape(h, w, -1)[zero] == 0).all() and not inside[zero].any()
    bad, excused, _ = R.classify_bytes(v, np.rint(v))
    assert not bad.any() and G.share(excused) <= G.CAP and not ((h, w) in G.THIN and excused.any())
    assert G.share(R.warp_valid_excused(sx, sy, h, w)) <= G.CAP and G.share(R.warp_nearest_excused(sx, sy, h, w)) <= G.CAP
    if (h, w) not in G.THIN:
        assert R.warp_valid64(sx, sy, h, w).any() and (v > 0).any()         # and the rest of the frame shows something
    v, sx, sy = R.warp_linear64(img, G.FAR)
    assert not v.any() and not R.warp_valid64(sx, sy, h, w).any() and not R.warp_nearest64(img, G.FAR)[0].any()
    assert not R.warp_valid_excused(sx, sy, h, w).any() and not R.warp_nearest_excused(sx, sy, h, w).any()


@pytest.mark.parametrize("c", G.CHANNELS)
@pytest.mark.parametrize("h,w", G.SIZES)
def test_exact_cases(h, w, c):
    """For integer and half-integer source coordinates the fp64 value is exact, so its rint (half to even) IS the byte: the
    integer-arithmetic expectation, the numpy-indexing expectation and the fp64 reference must agree byte for byte, and the
    fp32 oracle with them."""
    img = G.image(h, w, c)
    ones = np.ones((h, w), np.uint8)
    ties = {}
    for name, Hm, Hinv, sx2, sy2, by_numpy in G.exact_cases(h, w):
        assert np.array_equal(np.linalg.inv(Hm), Hinv), name
        v, sx, sy = R.warp_linear64(img, Hm)
        assert np.array_equal(2 * sx, sx2) and np.array_equal(2 * sy, sy2), name
        want, want_valid = R.warp_halves_exact(img, sx2, sy2)
        assert np.array_equal(np.rint(v), want), name
        assert np.array_equal(R.warp_valid64(sx, sy, h, w), want_valid), name
        assert np.array_equal(tracker_ref.warp_linear_u8(img, Hm), want), name
        near, near_inside = R.nearest_halves_exact(img, sx2, sy2)
        got_near, _, _, inside = R.warp_nearest64(img, Hm)
        assert np.array_equal(got_near, near) and np.array_equal(inside, near_inside), name
        if by_numpy is not None:
            assert np.array_equal(want, by_numpy(img)) and np.array_equal(near, by_numpy(img)), name
            assert np.array_equal(want_valid, by_numpy(ones).astype(bool)), name
            assert np.array_equal(near_inside, want_valid), name
        ties[name] = G.share(R.classify_bytes(v, want)[1])
    if (h, w) == (61, 83):                             # why the half-pixel cases are exact cases: a quarter of their bytes tie
        assert all(ties[f"half({tx},{ty})"] > 0.2 for tx, ty in G.HALF_SHIFTS), ties


def test_rint_div_rounds_half_to_even():
    s = np.arange(0, 4 * 255 + 1)
    for n in (2, 4, 16):
        assert np.array_equal(R.rint_div(s, n), np.rint(s / n).astype(np.int64))
    assert R.rint_div(np.array([2, 6, 10, 14]), 4).tolist() == [0, 2, 2, 4]


@pytest.mark.parametrize("factor", G.RESIZE_FACTORS)
@pytest.mark.parametrize("c", G.CHANNELS)
@pytest.mark.parametrize("h,w", G.RESIZE_SIZES)
def test_resize_reference(h, w, c, factor):
    """Every factor here gives weights that are multiples of 1/4, so v is a multiple of 1/16 below 256: exact in fp32 as in
    fp64, and the byte is rint(v), half to even, with no band (ties are structural here -- up to a quarter of the bytes -- so
    the rule alone would excuse too much).  The fp32 oracle must give exactly that."""
    img = G.image(h, w, c, seed=1)
    ho, wo = R.resize_out_shape(h, w, factor)
    v = R.resize_linear64(img, factor)
    assert v.shape == (ho, wo) + img.shape[2:] and v.dtype == np.float64
    assert np.array_equal(v * 16, np.rint(v * 16))
    got = tracker_ref.resize_linear_u8(img, factor)
    assert got.shape == v.shape
    assert not R.classify_bytes(v, got)[0].any() and np.array_equal(got, np.rint(v))
    if factor == 2 and h % 2 == 0 and w % 2 == 0:
        s = img.astype(np.int64).reshape(h // 2, 2, w // 2, 2, -1).sum((1, 3)).reshape(v.shape)
        assert np.array_equal(np.rint(v), R.rint_div(s, 4))


def test_resize_output_sizes_round_half_to_even():
    assert R.resize_out_shape(37, 45, 2) == (18, 22) and R.resize_out_shape(39, 47, 2) == (20, 24)
    assert R.resize_out_shape(1, 97, 2) == (0, 48) and R.resize_out_shape(1, 1, 1.5) == (1, 1)
    x = (np.arange(24) + 0.5) * 2 - 0.5
    assert np.floor(x)[-1] >= 47 - 1 - 1e-9            # 39x47 by 2: the last column starts at the last source column (the clamp)


def test_windowed_cases_hold_the_caps():
    """The conditions test_image_geometry_gpu puts on the 123x157 frame of the window tests."""
    h, w = 123, 157
    img = G.image(h, w, 3)
    for hname, Hm in G.GENERIC.items():
        v, sx, sy = R.warp_linear64(img, Hm)
        _, excused, _ = R.classify_bytes(v, np.rint(v))
        y0, x0, rows, cols = 31, 42, 57, 71
        assert G.share(excused[y0:y0 + rows, x0:x0 + cols]) <= G.CAP, hname
        assert not excused[h - 1, w - 1].any(), hname
        vex = R.warp_valid_excused(sx, sy, h, w)
        assert G.share(vex[y0:y0 + rows, x0:x0 + cols]) <= G.CAP and not vex[h - 1, w - 1], hname
