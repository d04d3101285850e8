"""CPU checks of the background and the photometric augmentation of the pair generator: the noise
definition against pinned values and its moments, the float64 host constructions (blur_taps, colour_matrix), the float64
restatement of tests/hsynth_aug_host.py, the ABI and the argument validation of both new entries (no launch: no GPU here)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import hsynth_aug_host as ah
import hsynth_host as hh

ROOT = Path(__file__).resolve().parent.parent
SEEDS = (0, 1, 12345, 2 ** 32 - 1)


# ---- the noise -------------------------------------------------------------------------------------------------------------------
def test_noise_pinned_values():
    """w = 4, h = 1, channel 0 of the first pixels... the definition's z at idx 0 .. 3 for seeds 0 and 1, recomputed from the
    integer definition."""
    want = {0: (-1.8990821, -0.791522, 1.7099297, 2.0392613), 1: (0.3905413, 0.7930285, -2.6858733, 1.7512118)}
    for seed, values in want.items():
        S = ah.noise_int(seed, np.arange(4))
        assert S.dtype == np.int64 and np.all(np.abs(S) <= 131070)
        z = (S.astype(np.float32) * ah.Z_SCALE).astype(np.float64)
        assert np.max(np.abs(z - np.array(values))) <= 1e-6, (seed, z)
        assert np.max(np.abs(ah.noise_z(seed, 1, 4).reshape(-1)[:4] - np.array(values))) <= 1e-6


def test_noise_index_wraps_at_32_bits():
    assert np.array_equal(ah.noise_int(7, np.array([5, 2 ** 32 + 5], dtype=np.uint64)), ah.noise_int(7, np.array([5, 5])))
    assert not np.array_equal(ah.noise_int(7, np.arange(8)), ah.noise_int(8, np.arange(8)))


@pytest.mark.parametrize("seed", SEEDS)
def test_noise_moments(seed):
    """A 64 x 64 x 3 constant frame with noise_sigma = 1: |mean| <= 4 / sqrt(12288), variance in [0.94, 1.06], |z| <= 3.47."""
    u = ah.augment(np.full((64, 64, 3), 100.0, np.float32), noise_sigma=1.0, seed=seed)
    z = u - 100.0
    assert abs(float(z.mean())) <= 4.0 / np.sqrt(12288.0), z.mean()
    assert 0.94 <= float(z.var()) <= 1.06, z.var()
    assert float(np.abs(z).max()) <= ah.Z_MAX
    for shifted in (z[1:] * z[:-1], z[:, 1:] * z[:, :-1], z[..., 1:] * z[..., :-1]):       # neighbours down, across, in channel
        assert abs(float(shifted.mean())) <= 0.05


# ---- host constructions ----------------------------------------------------------------------------------------------------------
def test_blur_taps():
    from woft_amd.hsynth import blur_taps
    assert blur_taps(0.0).tolist() == [1.0]
    for sigma, radius in ((0.3, 1), (0.34, 2), (1.0, 3), (2.0, 6), (2.5, 7), (10.0, 7)):
        t = blur_taps(sigma)
        assert t.dtype == np.float32 and t.shape == (2 * radius + 1,), (sigma, t.shape)
        assert abs(float(t.astype(np.float64).sum()) - 1.0) <= 1e-7
        assert np.array_equal(t, t[::-1]) and np.all(t > 0) and t[radius] == t.max()
    assert all((len(blur_taps(s)) - 1) // 2 == r for r, s in ah.SIGMA_OF_RADIUS.items())
    with pytest.raises(ValueError, match="blur_sigma"):
        blur_taps(-1.0)


def test_colour_matrix():
    from woft_amd.hsynth import colour_matrix
    M, o = colour_matrix(1.0, 0.0, 1.0)
    assert M.dtype == np.float64 and np.array_equal(M, np.eye(3)) and np.array_equal(o, np.zeros(3))
    grey = np.array([93.0, 93.0, 93.0])
    for hue in (0.3, -1.1, np.pi):
        M, o = colour_matrix(1.0, hue, 1.0)
        assert np.max(np.abs(M @ grey + o - grey)) <= 1e-4
        assert np.max(np.abs(M @ M.T - np.eye(3))) <= 1e-12          # a rotation
    M, o = colour_matrix(0.0, 0.0, 1.0)                              # no saturation: every channel the grey
    x = np.array([10.0, 200.0, 90.0])
    assert np.max(np.abs(M @ x + o - (0.114 * 10 + 0.587 * 200 + 0.299 * 90))) <= 1e-12
    M, o = colour_matrix(1.0, 0.0, 1.5)                              # contrast about 127.5
    assert np.allclose(M @ np.full(3, 127.5) + o, 127.5) and np.allclose(M @ np.full(3, 137.5) + o, 142.5)
    M, o = colour_matrix(0.7, 0.4, 1.2)                              # grey stays grey through all three
    assert np.max(np.abs(M @ grey + o - (1.2 * (93.0 - 127.5) + 127.5))) <= 1e-9


# ---- restatement sanity ------------------------------------------------------------------------------------------------------------
def test_blur_restatement():
    rs = np.random.RandomState(3)
    f = rs.uniform(0, 255, (9, 11, 3))
    from woft_amd.hsynth import blur_taps
    for sigma in (0.3, 2.5):
        taps = blur_taps(sigma)
        r = (len(taps) - 1) // 2
        got = ah.blur(f, taps)
        pad = np.pad(f, ((r, r), (r, r), (0, 0)), mode="edge")
        want = np.zeros_like(f)
        for j in range(2 * r + 1):
            for i in range(2 * r + 1):
                want += float(taps[j]) * float(taps[i]) * pad[j:j + 9, i:i + 11]
        assert np.max(np.abs(got - want)) <= 1e-10
        assert np.max(np.abs(ah.blur(np.full((5, 4, 3), 77.0), taps) - 77.0)) <= 1e-4


def test_background_restatement():
    base = hh.base_image()
    bg = ah.backgrounds()["11x7"]
    out_hw = (17, 33)
    H = hh.homographies(out_hw)["random0"]
    # where the plane covers a pixel wholly the background does not show; with no background pixel (all zeros) it is render
    v, cover, P = ah.render_bg(base, H, np.zeros((2, 2, 3), np.uint8), np.eye(3), out_hw=out_hw)
    assert np.max(np.abs(v - hh.render(base, H, out_hw=out_hw)[0])) == 0.0 and 0 < P.mean() < 1 and np.all(cover == 0)
    # a plane wholly outside: the background alone, and a constant background is that constant everywhere
    away = np.array([[1.0, 0.0, 1000.0], [0.0, 1.0, 1000.0], [0.0, 0.0, 1.0]])
    one = ah.backgrounds()["1x1"]
    v, _, P = ah.render_bg(base, away, one, ah.background_H(one, out_hw), out_hw=out_hw)
    assert np.all(P == 0) and np.max(np.abs(v - one[0, 0].astype(np.float64))) <= 1e-9
    # the identity background homography reads the background's own pixels, replicated beyond it
    v, _, _ = ah.render_bg(base, away, bg, np.eye(3), out_hw=out_hw)
    assert np.array_equal(v[:11, :7], bg.astype(np.float64)) and np.array_equal(v[16, 32], bg[10, 6].astype(np.float64))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_abi(lib):
    import woft_amd
    from woft_amd import _lib, hsynth
    header = (ROOT / "include" / "woft_hip.h").read_text()
    for name in ("woft_hsynth_render_bg", "woft_hsynth_augment"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"^\s*int\s+" + name + r"\s*\(", header, flags=re.M)
    assert "WOFT_HSYNTH_MAX_BLUR 7" in header and hsynth.MAX_BLUR == 7
    assert lib.woft_abi_version() == 400
    for name in ("augment", "blur_taps", "colour_matrix"):
        assert getattr(woft_amd, name) is getattr(hsynth, name)


def test_argument_validation_without_gpu(lib):
    """Every rejected argument returns -1 before any launch (the pointers are never dereferenced on the device: no GPU here)."""
    from woft_amd import _lib
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p).value                       # a non-NULL, 4-byte aligned address
    H = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    occ = (_lib.HSynthOccluder * 5)()
    for o in occ:
        o.tex, o.ho, o.wo = p, 2, 2

    def render_bg(base=p, hs=8, ws=8, hinv=H, occ_=occ, n=1, bg=p, hb=4, wb=4, hinv_bg=H, out=p, h=8, w=8):
        return lib.woft_hsynth_render_bg(base, hs, ws, hinv, None, None, occ_, n, bg, hb, wb, hinv_bg, out, None, None, None, h, w,
                                         None)

    for bad in (dict(bg=None), dict(hinv_bg=None), dict(hb=0), dict(wb=-1), dict(hb=1 << 16, wb=1 << 15),
                # the old list
                dict(base=None), dict(hinv=None), dict(out=None), dict(hs=0), dict(ws=-1), dict(h=0), dict(w=0), dict(n=-1),
                dict(n=5), dict(occ_=None), dict(hs=1 << 16, ws=1 << 15), dict(h=1 << 15, w=1 << 16)):
        assert render_bg(**bad) == -1, bad
    for field, value in (("tex", None), ("tex", p + 1), ("ho", 0), ("wo", -2)):
        one = (_lib.HSynthOccluder * 2)()
        for o in one:
            o.tex, o.ho, o.wo = p, 2, 2
        setattr(one[1], field, value)
        assert render_bg(occ_=one, n=2) == -1, field

    taps = (C.c_float * 15)(*([1.0 / 15] * 15))
    q = p + 16

    def augment(inp=p, h=8, w=8, taps_=taps, radius=1, sigma=0.0, out_u8=q, out_f32=None):
        return lib.woft_hsynth_augment(inp, h, w, taps_, radius, None, sigma, 0, out_u8, out_f32, None)

    for bad in (dict(inp=None), dict(out_u8=None), dict(h=0), dict(w=-2), dict(h=1 << 15, w=1 << 16), dict(radius=-1),
                dict(radius=8), dict(taps_=None), dict(out_f32=p), dict(radius=7, out_f32=p), dict(sigma=-0.5),
                dict(sigma=float("nan")), dict(sigma=float("inf")), dict(radius=0, sigma=-1.0)):
        assert augment(**bad) == -1, bad
