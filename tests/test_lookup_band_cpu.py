"""The correlation band's geometry and hit rule, mirrored in pure Python (woft_amd/ops.py: band_m, band_geometry, band_hit) and
checked by brute force: whenever the predicate holds, every cell of every level's (2r + 2)^2 window lies inside the stored band;
the margins are the smallest that keep a level-0 displacement within [-m_0, m_0] cells inside the band at every level; and the
library's own numbers (woft_corr_band_geometry, the macros of include/woft_hip.h) equal the mirrored ones."""
import ctypes as C
import math

import numpy as np
import pytest

from woft_amd import _lib, ops


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _window_cells(c, p, r, l):
    """Cells of one axis of the lookup window of level l for the coordinate c, and of the band of source position p."""
    o = math.floor(c / (1 << l)) - r
    win = range(o, o + 2 * r + 2)
    m = ops.band_m(l)
    b0 = (p >> l) - r - m
    return win, range(b0, b0 + 2 * (r + 1 + m))


@pytest.mark.parametrize("r", [4, 3])
def test_predicate_implies_every_window_cell_is_stored(r):
    """Source positions 0 .. 40 on both axes of a map with a ragged border; coordinates p + d for d over integers, half-integers,
    quarter steps and one float around every integer, from beyond -m_0 - 1 to beyond m_0 + 2 -- negative coordinates near the
    border included.  Predicate true => all window cells inside the band, on every level; and conversely a window that fits on
    every level is never called a miss."""
    steps = sorted({float(np.float32(v)) for k in range(-6, 8) for v in
                    (k, k + 0.25, k + 0.5, k + 0.75, np.nextafter(np.float32(k), np.float32(-np.inf)),
                     np.nextafter(np.float32(k), np.float32(np.inf)))})
    n_hit = n_miss = 0
    for p in range(0, 41):
        for d in steps:
            c = float(np.float32(p + d))
            fits = True
            for l in range(4):
                win, band = _window_cells(c, p, r, l)
                fits &= win[0] >= band[0] and win[-1] <= band[-1]
            hit = ops.band_hit(c, c, p, p, 4)
            assert hit == fits, (p, d, c)
            n_hit, n_miss = n_hit + hit, n_miss + (not hit)
            if -ops.BAND_M0 <= c - p < ops.BAND_M0:                  # the displacements the band is built for
                assert hit, (p, d)
    assert n_hit > 1000 and n_miss > 1000


def test_margins_are_the_smallest_that_hold_the_level0_band():
    """m_l = ceil(m_0 / 2^l): for some position the centre cell really moves by -m_l and by +m_l while the level-0 displacement
    stays within [-m_0, m_0], and never further."""
    for l in range(4):
        lo = min(math.floor((p + d) / (1 << l)) - (p >> l) for p in range(64) for d in (-ops.BAND_M0, ops.BAND_M0))
        hi = max(math.floor((p + d) / (1 << l)) - (p >> l) for p in range(64) for d in (-ops.BAND_M0, ops.BAND_M0))
        assert (lo, hi) == (-ops.band_m(l), ops.band_m(l)) and ops.band_m(l) == -(-ops.BAND_M0 // (1 << l))


def test_library_geometry_equals_the_mirror(lib):
    for r, levels in ((4, 4), (3, 4), (4, 2), (3, 1)):
        m, w, off = (np.zeros(4, np.int32) for _ in range(3))
        i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        rows = lib.woft_corr_band_geometry(r, levels, i32p(m), i32p(w), i32p(off))
        assert (list(m[:levels]), list(w[:levels]), list(off[:levels]), rows) == ops.band_geometry(r, levels)
        assert max(w) <= ops.BAND_LD
    assert ops.band_geometry(4, 4) == ([3, 2, 1, 1], [16, 14, 12, 12], [0, 16, 30, 42], 54)      # 3456 bytes per source pixel
    assert lib.woft_corr_band_geometry(5, 4, None, None, None) == -1                              # W_0 would exceed a row
    assert lib.woft_corr_band_geometry(4, 5, None, None, None) == -1
    assert lib.woft_sizeof(3) == C.sizeof(_lib.LookupBandParams)


def test_entry_points_reject_bad_arguments_without_a_launch(lib):
    """NULL band / flags / counter, exact fp32 (terms 0), a (radius, k) without an instance, a rectangle outside the map: -1
    before anything is launched (the pointers are host addresses no launch may see)."""
    buf = (C.c_float * 1024)()
    a = C.addressof(buf)

    def params(**kw):
        p = _lib.LookupBandParams()
        o = p
        o.f1 = a
        for l in range(4):
            o.f2[l], o.h[l], o.w[l] = a, max(16 >> l, 1), max(24 >> l, 1)
        o.levels, o.radius, o.terms, o.hf, o.wf, o.k, o.alpha = 4, 4, 3, 16, 24, 256, 1 / 16
        o.coords, o.out, o.ldo = a, a, 324
        p.band, p.miss, p.miss_count = a, a, a
        for name, v in kw.items():
            setattr(p, name, v)
        return p
    for bad in (dict(band=None), dict(terms=0), dict(terms=2), dict(radius=3), dict(k=128), dict(levels=0), dict(levels=5),
                dict(f1=None), dict(ablate=1)):
        assert lib.woft_corr_band_build(C.byref(params(**bad)), None) == -1, bad
    for bad in (dict(band=None), dict(miss=None), dict(miss_count=None), dict(terms=0), dict(radius=3), dict(ldo=323),
                dict(coords=None), dict(out=None), dict(roi_y0=12, roi_h=8, roi_w=8), dict(smp_x0=20, smp_h=8, smp_w=8),
                dict(ablate=1), dict(fh_part=a)):
        assert lib.woft_corr_lookup_band(C.byref(params(**bad)), None) == -1, bad
    assert lib.woft_corr_band_build(None, None) == -1 and lib.woft_corr_lookup_band(None, None) == -1
