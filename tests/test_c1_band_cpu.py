"""woft_conv1x1_band and woft_lookup_band_params.defer_samples without a GPU: the struct mirror has the library's size, the entry
point is exported, and it answers -1 before any launch for NULL arguments, an instance it is not built for, mismatched precisions
and a partner that cannot share the launch (the pointers are host addresses no launch may see)."""
import ctypes as C

import pytest

from woft_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_struct_mirror_and_export(lib):
    assert lib.woft_sizeof(3) == C.sizeof(_lib.LookupBandParams)
    assert "woft_conv1x1_band" in _lib.EXPORTS and hasattr(lib, "woft_conv1x1_band")
    fields = [n for n, _ in _lib.LookupBandParams._fields_]
    assert fields[-4:] == ["band", "miss", "miss_count", "defer_samples"]
    assert _lib.LookupBandParams().defer_samples == 0            # (a struct built as before asks for what it always got)


def _args(a):
    """The 16 x 24 instance the entry point takes, on host addresses: (convc1, convf1, band parameters)."""
    bp = _lib.LookupBandParams()
    bp.f1 = a
    for l in range(4):
        bp.f2[l], bp.h[l], bp.w[l] = a, max(16 >> l, 1), max(24 >> l, 1)
    bp.levels, bp.radius, bp.terms, bp.hf, bp.wf, bp.k, bp.alpha = 4, 4, 3, 16, 24, 256, 1 / 16
    bp.coords, bp.out, bp.ldo = a, a, 352
    bp.band, bp.miss, bp.miss_count = a, a, a

    def conv(**kw):
        p = _lib.ConvParams()
        p.in0, p.n_img, p.h, p.w, p.ho, p.wo = a, 1, 16, 24, 16, 24
        p.taps_x, p.stride, p.wgt, p.wgt_hi, p.wgt_lo, p.wgt_frag, p.precision = 1, 1, a, a, a, a, 1
        p.bias, p.alpha, p.out, p.epi, p.tile_m, p.halo = a, 1.0, a, _lib.EPI_RELU, 64, 16
        for name, v in kw.items():
            setattr(p, name, v)
        return p
    c1 = conv(cs0=352, c_split=352, taps_y=1, cin_pad=352, cout=256, cout_pad=256, ldo=256, tile_n=256)
    f1 = conv(cs0=4, c_split=32, taps_y=7, pad_y=3, pad_x=3, cin_pad=32, flat=1, cout=128, cout_pad=128, ldo=128, tile_n=128)
    return c1, f1, bp


def test_entry_point_rejects_bad_arguments_without_a_launch(lib):
    buf = (C.c_float * 1024)()
    a = C.addressof(buf)

    def call(edit=None, partner=True, **null):
        c1, f1, bp = _args(a)
        if edit is not None:
            edit(c1, f1, bp)
        r = lambda p, name: None if null.get(name) else C.byref(p)
        return lib.woft_conv1x1_band(r(c1, "c1"), r(f1, "f1") if partner else None, r(bp, "bp"), None)

    assert call(c1=True) == -1 and call(bp=True) == -1 and call(c1=True, bp=True, partner=False) == -1

    def setter(which, **kw):
        def edit(c1, f1, bp):
            for name, v in kw.items():
                setattr({"c1": c1, "f1": f1, "bp": bp}[which], name, v)
        return edit
    bad = [
        setter("bp", band=None), setter("bp", coords=None),
        setter("bp", k=128, radius=3), setter("bp", k=128), setter("bp", radius=3), setter("bp", levels=3), setter("bp", terms=0),
        setter("bp", need=a), setter("bp", ablate=1), setter("bp", roi_y0=8, roi_h=8, roi_w=8), setter("bp", smp_h=8, smp_w=8),
        setter("bp", ldo=356), setter("bp", out=a + 16),                         # (not convc1's input buffer)
        setter("c1", cout=96, cout_pad=128, tile_n=128), setter("c1", cin_pad=320, c_split=320),
        setter("c1", h=8, ho=8), setter("c1", n_img=2), setter("c1", halo=0), setter("c1", precision=0), setter("c1", precision=4),
        setter("c1", wgt_frag=None), setter("c1", roi_y0=0, roi_x0=0, roi_h=8, roi_w=8), setter("c1", epi=_lib.EPI_CTX),
        setter("f1", precision=2), setter("c1", precision=3),                   # mismatched precisions
        setter("f1", flat=0, taps_y=1, pad_y=0, pad_x=0, cs0=32),               # partners that cannot share the launch
        setter("f1", halo=8), setter("f1", tile_n=64), setter("f1", taps_y=5), setter("f1", roi_h=8, roi_w=8),
        setter("f1", wgt_frag=None), setter("f1", h=8, ho=8, stride=2),
    ]
    for k, edit in enumerate(bad):
        assert call(edit) == -1, k
    # (without a partner the same instance checks apply)
    assert call(setter("c1", cout=96, cout_pad=128, tile_n=128), partner=False) == -1
    assert call(setter("bp", k=128, radius=3), partner=False) == -1
