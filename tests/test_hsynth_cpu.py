"""CPU checks of the synthetic-homography pair generator: the float64 restatement the GPU tests compare
against (tests/hsynth_host.py), the host-side draws, the ABI and its argument validation, and the margins that let the GPU label
test ask for equality."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import hsynth_host as hh

ROOT = Path(__file__).resolve().parent.parent


# ---- restatement sanity ------------------------------------------------------------------------------------------------------------
def test_identity_labels():
    flow, visible, valid = hh.labels((24, 40), np.eye(3))
    assert np.all(flow == 0.0) and np.all(visible == 1.0) and np.all(valid)


def test_render_equals_warp_image_np():
    from woft_amd import synth
    base = hh.base_image()
    for out_hw in (None, (17, 33)):
        for H in hh.homographies(out_hw or hh.BASE_HW).values():
            got, cover = hh.render(base, H, out_hw=out_hw)
            assert np.max(np.abs(got - synth.warp_image_np(base, H, out_hw=out_hw))) <= 1e-9
            assert np.all(cover == 0.0)


def test_direction_pin():
    """Render and labels use H_gt the same way round: following the flow from a visible template pixel finds that pixel's
    (photometrically changed) value in the rendered frame, to 1e-9: for every template pixel with visible == 1 that lands at least
    one pixel inside the frame -- less the two kinds of pixel at which the rendered frame is by definition not 1.5 * base + 7:
    those whose four taps in the frame touch the warped image's own zero border, and those whose taps an occluder's footprint
    reaches (visible == 1 allows a coverage of up to lo)."""
    h, w = 40, 60
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    ramp = xs + 2.0 * ys                                      # <= 59 + 78: fits uint8
    base = np.repeat(ramp[..., None], 3, 2).astype(np.uint8)
    H = np.array([[0.9, 0.12, 3.3], [-0.08, 1.05, 2.1], [0.0, 0.0, 1.0]])          # affine: bilinear sampling of a ramp is exact
    tex = hh.textures()[3]
    occ = [(tex, hh._place(1.3, 0.4, 31.2, 17.7, tex))]
    img, _ = hh.render(base, H, occ, gain=1.5, bias=7.0)
    flow, visible, valid = hh.labels((h, w), H, occ)
    px, py = xs + flow[0], ys + flow[1]
    sel = (visible == 1.0) & (px >= 1) & (px <= w - 2) & (py >= 1) & (py <= h - 2)
    # (the base image is zero outside itself: keep the pixels whose four taps in the frame all see the ramp, not its border)
    Hi = np.linalg.inv(H)
    for dx in (0, 1):
        for dy in (0, 1):
            qx, qy = np.floor(px) + dx, np.floor(py) + dy
            sx, sy = Hi[0, 0] * qx + Hi[0, 1] * qy + Hi[0, 2], Hi[1, 0] * qx + Hi[1, 1] * qy + Hi[1, 2]
            sel &= (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    assert sel.sum() > 500 and (visible == 0.0).sum() > 50
    got = hh.sample_bilinear(img, px, py)[sel]
    want = (1.5 * ramp + 7.0)[sel]
    # the occluder's own bilinear footprint reaches one destination pixel beyond T > 0: drop taps it touches
    cov = hh.sample_bilinear(hh.render(base, H, occ)[1][..., None], px, py)[..., 0][sel]
    ok = cov == 0.0
    assert ok.sum() > 500
    assert np.max(np.abs(got[ok] - want[ok][:, None])) <= 1e-9


# ---- host-side draws ---------------------------------------------------------------------------------------------------------------
def test_random_homography_determinism_and_convexity():
    from woft_amd.hsynth import _strictly_convex, random_homography
    a = random_homography(np.random.RandomState(5), 120, 160)
    b = random_homography(np.random.RandomState(5), 120, 160)
    c = random_homography(np.random.RandomState(6), 120, 160)
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert a.dtype == np.float64 and a.shape == (3, 3) and a[2, 2] == 1.0
    rs = np.random.RandomState(7)
    corners = np.array([[0.0, 0.0, 1.0], [159.0, 0.0, 1.0], [159.0, 119.0, 1.0], [0.0, 119.0, 1.0]])
    for _ in range(200):
        H = random_homography(rs, 120, 160, max_shift=0.45)
        q = corners @ H.T
        assert np.all(q[:, 2] > 0)
        q = q[:, :2] / q[:, 2:]
        assert _strictly_convex(q)
        assert np.max(np.abs(q - corners[:, :2])) <= 0.45 * 120 + 1e-9


def test_make_occluder():
    from woft_amd.hsynth import make_occluder
    for seed in range(6):
        t = make_occluder(np.random.RandomState(seed), 21, 35)
        assert t.shape == (21, 35, 4) and t.dtype == np.uint8
        assert set(np.unique(t[..., 3])) <= {0, 255} and (t[..., 3] == 255).sum() > 50
        assert t.tobytes() == make_occluder(np.random.RandomState(seed), 21, 35).tobytes()


def test_hsynth_refuses_wrong_inputs():
    from woft_amd.hsynth import HSynth, random_homography
    with pytest.raises(ValueError, match=r"images\[0\].*multiples of 8"):
        HSynth([np.zeros((130, 160, 3), np.uint8)])
    with pytest.raises(TypeError, match=r"images\[0\]"):
        HSynth([np.zeros((128, 160, 3), np.float32)])
    with pytest.raises(ValueError, match=r"images\[0\]"):
        HSynth([np.zeros((128, 160), np.uint8)])
    with pytest.raises(TypeError, match="rs"):
        random_homography(3, 120, 160)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_abi(lib):
    from woft_amd import _lib
    header = (ROOT / "include" / "woft_hip.h").read_text()
    for name in ("woft_hsynth_render", "woft_hsynth_labels"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"^\s*int\s+" + name + r"\s*\(", header, flags=re.M)
    assert "WOFT_HSYNTH_MAX_OCC 4" in header
    assert lib.woft_abi_version() == 400
    assert lib.woft_sizeof(4) == C.sizeof(_lib.HSynthOccluder) == 96


def test_argument_validation_without_gpu(lib):
    """Every rejected argument returns -1 before any launch (the pointers are never dereferenced on the device: no GPU here)."""
    from woft_amd import _lib
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p).value                       # a non-NULL, 4-byte aligned address
    H = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    occ = (_lib.HSynthOccluder * 5)()
    for o in occ:
        o.tex, o.ho, o.wo = p, 2, 2

    def render(base=p, hs=8, ws=8, hinv=H, occ_=occ, n=1, out=p, h=8, w=8):
        return lib.woft_hsynth_render(base, hs, ws, hinv, None, None, occ_, n, out, None, None, h, w, None)

    def labels(hs=8, ws=8, hf=H, occ_=occ, n=1, h=8, w=8, lo=0.25, hi=0.75, flow=p, vis=p, valid=p):
        return lib.woft_hsynth_labels(hs, ws, hf, occ_, n, h, w, lo, hi, flow, vis, valid, None)

    for bad in (dict(base=None), dict(hinv=None), dict(out=None), dict(hs=0), dict(ws=-1), dict(h=0), dict(w=0), dict(n=-1),
                dict(n=5), dict(occ_=None), dict(hs=1 << 16, ws=1 << 15), dict(h=1 << 15, w=1 << 16)):
        assert render(**bad) == -1, bad
    for bad in (dict(hf=None), dict(flow=None), dict(vis=None), dict(valid=None), dict(hs=0), dict(ws=0), dict(h=-3), dict(w=0),
                dict(n=-1), dict(n=5), dict(occ_=None), dict(hs=1 << 16, ws=1 << 15), dict(h=1 << 15, w=1 << 16),
                dict(lo=-0.1), dict(lo=0.5, hi=0.5), dict(lo=0.8, hi=0.7), dict(hi=1.5), dict(lo=float("nan"))):
        assert labels(**bad) == -1, bad
    for field, value in (("tex", None), ("tex", p + 1), ("ho", 0), ("wo", -2)):
        one = (_lib.HSynthOccluder * 2)()
        for o in one:
            o.tex, o.ho, o.wo = p, 2, 2
        setattr(one[1], field, value)
        assert render(occ_=one, n=2) == -1 and labels(occ_=one, n=2) == -1, field


# ---- the condition the GPU label test relies on ----------------------------------------------------------------------------------
def test_label_margins():
    """In float64 no template pixel of the GPU label test's inputs is within 1e-4 of a threshold in T, within 1e-6 of the frame's
    border in px / py, or within 1e-3 of the horizon in d: float32 / fp64 rounding on the device cannot flip a label.  (With the
    identity px = x and py = y hold exactly in any IEEE arithmetic -- one multiplication by 1, additions of 0, a division by 1 --
    so the border, which the identity hits by construction, needs no margin there; T and d keep theirs.)"""
    seen = {"horizon": False, "soft": False, "hidden": False, "outside": False}
    for name, H, occ, (h, w) in hh.label_cases():
        flow, visible, valid, (px, py, d, T, inside) = hh.labels(hh.BASE_HW, H, occ, out_hw=(h, w), detail=True)
        assert np.min(np.abs(d)) >= 1e-3, name
        pos = d > 0
        if not np.array_equal(H, np.eye(3)):
            for v, edge in ((px, 0.0), (px, w - 1.0), (py, 0.0), (py, h - 1.0)):
                assert np.min(np.abs(v[pos] - edge)) >= 1e-6, name
        Tin = T[inside]
        assert np.all(np.isfinite(Tin)), name
        assert Tin.size == 0 or min(np.min(np.abs(Tin - 0.25)), np.min(np.abs(Tin - 0.75))) >= 1e-4, name
        seen["horizon"] |= bool((~pos).any() and pos.any())
        seen["soft"] |= bool((~valid).any())
        seen["hidden"] |= bool((inside & (visible == 0.0) & valid).any())
        seen["outside"] |= bool((~inside).any())
    assert all(seen.values()), seen
