"""The per-frame image-geometry kernels against float64 references, byte by byte: the perspective warp (bilinear, nearest, validity
mask; csrc/warp_pixel.h) in its full-frame, windowed and fused mask-and-box forms, the input downscale and the rectangle copy.

A bilinear byte must be rint of the fp64 value unless that value lies within fp64_refs.WARP_BAND (derived there from the
kernel's fp32 roundings) of a .5 tie; a validity or nearest byte must be the reference's unless the source coordinate sits on the
frame's border / on a half-integer to within fp64 rounding.  Each generic case asserts that it excuses at most G.CAP of its
bytes.  Homographies whose source coordinates are integers and half-integers are exact in fp32 and are held to every byte.
Every output is a view into a sentinel buffer with guard bytes on both sides, each kernel runs with `out` alone, `valid` alone and
both, over two different pre-fills: the results must agree (so every byte was written) and the guards must survive.
tests/test_image_geometry_cpu.py proves the conditions on the inputs, and the rule itself on the fp32 oracle, without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tracker_ref  # noqa: E402  (checker only)
from woft_amd import _lib, ops  # noqa: E402
import fp64_refs as R  # noqa: E402
import geometry_cases as G  # noqa: E402
from test_window_kernels_gpu import H as WIN_H, W as WIN_W, WINDOWS  # noqa: E402

GUARD = 64
FILLS = (77, 178)
EINVAL = -1


class Guarded:
    """An output of `shape` as a view `offset` bytes past a 4-byte boundary into a buffer pre-filled with `fill`, GUARD bytes of
    it before and after."""

    def __init__(self, shape, fill, offset=0):
        self.shape, self.fill, self.n, self.lo = tuple(shape), fill, int(np.prod(shape)), GUARD + offset
        self.buf = torch.full((self.lo + self.n + GUARD,), fill, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 4 == 0
        self.view = self.buf[self.lo:self.lo + self.n].view(self.shape)

    def numpy(self):
        """The output's bytes, after asserting that nothing around them was written."""
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == self.fill).all() and (b[self.lo + self.n:] == self.fill).all(), "guard bytes overwritten"
        return b[self.lo:self.lo + self.n].reshape(self.shape).copy()


def _all_ways(launch, shape, nearest):
    """launch(out, valid) with `out` alone (pre-fill 77), `valid` alone (bilinear only; 77) and both (178): the same bytes each
    time, hence every byte written; guards intact.  -> (out, valid) as numpy."""
    hw = shape[:2]
    a = Guarded(shape, FILLS[0])
    launch(a.view, None)
    b, bv = Guarded(shape, FILLS[1]), Guarded(hw, FILLS[1])
    launch(b.view, bv.view)
    out, out_b, valid = a.numpy(), b.numpy(), bv.numpy()
    assert np.array_equal(out, out_b), "out alone != out with valid"
    assert np.isin(valid, (0, 1)).all()
    if not nearest:
        cv = Guarded(hw, FILLS[0])
        launch(None, cv.view)
        assert np.array_equal(cv.numpy(), valid), "valid alone != valid with out"
    return out, valid


def _warp(img, Hm, nearest):
    t = torch.from_numpy(np.array(img)).cuda()
    return _all_ways(lambda o, v: ops.warp_perspective_u8(t, Hm, o, v, nearest=nearest), img.shape, nearest)


@functools.lru_cache(maxsize=None)
def _ref(hname, h, w, c):
    """The references of one non-exact case, computed once."""
    img, Hm = G.case_image(hname, h, w, c), G.homography(hname, h, w)
    v, sx, sy = R.warp_linear64(img, Hm)
    near, _, _, inside = R.warp_nearest64(img, Hm)
    ref = dict(img=img, Hm=Hm, v=v, sx=sx, sy=sy, d=R.warp_source64(h, w, Hm)[2], near=near, inside=inside,
               valid=R.warp_valid64(sx, sy, h, w), vex=R.warp_valid_excused(sx, sy, h, w),
               nex=R.warp_nearest_excused(sx, sy, h, w))
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _check_rule(what, v, got, thin=False):
    bad, excused, used = R.classify_bytes(v, got)
    print(f"GEOM {what}: bytes {got.size} excused {int(excused.sum())} ({100 * G.share(excused):.4f} %) used-the-band "
          f"{int(used.sum())} outside-the-rule {int(bad.sum())}")
    assert G.share(excused) <= G.CAP and not (thin and excused.any()), what
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), v[bad][:4], got[bad][:4])


def _check_flags(what, want, got, excused, thin=False):
    print(f"GEOM {what}: pixels {got.size} excused {int(excused.sum())} ({100 * G.share(excused):.4f} %) differing "
          f"{int((want != got).sum())}")
    assert G.share(excused) <= G.CAP and not (thin and excused.any()), what
    keep = ~excused
    assert np.array_equal(got[keep], want[keep]), (what, np.argwhere((got != want) & keep)[:4].tolist())


NONEXACT = list(G.GENERIC) + ["dzero", "far"]


@pytest.mark.parametrize("mode", ["bilinear", "nearest", "valid"])
@pytest.mark.parametrize("hname", NONEXACT)
@pytest.mark.parametrize("c", G.CHANNELS)
@pytest.mark.parametrize("h,w", G.SIZES)
def test_warp_against_fp64(h, w, c, hname, mode):
    ref, thin, what = _ref(hname, h, w, c), (h, w) in G.THIN, f"warp-{mode} {hname} {h}x{w}x{c}"
    out, valid = _warp(ref["img"], ref["Hm"], mode == "nearest")
    zero = ref["d"] == 0
    if hname == "horizon-inv" and (h, w) in G.CROSSED:
        assert (ref["d"] > 0).any() and (ref["d"] < 0).any()               # the reference really sees both signs of d
    if hname == "dzero":
        assert np.array_equal(np.linalg.inv(ref["Hm"]), G.dzero(h, w)[1]) and zero.any()
        assert not out.reshape(h, w, -1)[zero].any() and not valid[zero].any()          # d == 0.0: value 0, invalid
    if hname == "far":
        assert not out.any() and not valid.any()
    if mode == "bilinear":
        _check_rule(what, ref["v"], out, thin)
    elif mode == "valid":
        _check_flags(what, ref["valid"], valid.astype(bool), ref["vex"], thin)
    else:
        keep = ~ref["nex"]
        _check_flags(what, ref["inside"], valid.astype(bool), ref["nex"], thin)
        assert np.array_equal(out.reshape(h, w, -1)[keep], ref["near"].reshape(h, w, -1)[keep]), what


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("c", G.CHANNELS)
@pytest.mark.parametrize("h,w", G.SIZES)
def test_warp_exact_cases(h, w, c, mode):
    """Integer and half-pixel translations, flips, turns and the up-scale by 2: every fp32 operation of the kernel is exact, so
    every byte and every validity flag must be the integer-arithmetic expectation (ties half to even: rintf's rule, and the zero
    border at weight 1/2), and numpy's slice / flip / rot90 where there is one.  Nearest under half-pixel translations takes the
    even neighbour, rint's choice; parity with OpenCV's own tie rule remains unpinned, as oracle/tracker_ref.py says."""
    img, ones = G.image(h, w, c), np.ones((h, w), np.uint8)
    for name, Hm, Hinv, sx2, sy2, by_numpy in G.exact_cases(h, w):
        assert np.array_equal(np.linalg.inv(Hm), Hinv), name                # what ops hands to the kernel is exact
        out, valid = _warp(img, Hm, mode == "nearest")
        want, want_valid = R.warp_halves_exact(img, sx2, sy2) if mode == "bilinear" else R.nearest_halves_exact(img, sx2, sy2)
        assert np.array_equal(out, want), (name, int((out != want).sum()))
        assert np.array_equal(valid.astype(bool), want_valid), name
        if by_numpy is not None:
            assert np.array_equal(out, by_numpy(img)) and np.array_equal(valid, by_numpy(ones)), name


# ---- the windowed and the fused forms -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hname", list(G.GENERIC))
def test_windowed_warp_against_fp64(hname):
    """The windowed kernel held to warp_linear64 directly (not through the full-frame kernel) on two windows of the 123x157
    frame of test_window_kernels_gpu."""
    h, w, c = WIN_H, WIN_W, 3
    ref = _ref(hname, h, w, c)
    t = torch.from_numpy(np.array(ref["img"])).cuda()
    for wname in ("inner", "one-pixel"):
        y0, x0, rows, cols = WINDOWS[wname]
        sl = (slice(y0, y0 + rows), slice(x0, x0 + cols))
        out, valid = _all_ways(lambda o, v: ops.warp_perspective_window_u8(t, ref["Hm"], WINDOWS[wname], o, v), (rows, cols, c),
                               False)
        _check_rule(f"window-bilinear {hname} {wname}", ref["v"][sl], out, thin=wname == "one-pixel")
        _check_flags(f"window-valid {hname} {wname}", ref["valid"][sl], valid.astype(bool), ref["vex"][sl], wname == "one-pixel")


def _np_bbox(m):
    ys, xs = np.nonzero(m)
    return [int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max()), 1] if ys.size else [0, 0, 0, 0, 0]


MASK_CASES = NONEXACT + [f"shift({tx},{ty})" for tx, ty in G.INT_SHIFTS]


@pytest.mark.parametrize("hname", MASK_CASES)
@pytest.mark.parametrize("h,w", G.SIZES)
def test_fused_mask_warp_against_fp64(h, w, hname):
    """ops.mask_bbox(mask, Hmat=...): the warped mask against warp_nearest64, the box against numpy on the reference's mask
    wherever no pixel is excused (always so for the integer translations and `far`), the scratch left zeroed."""
    Hm = dict((n, m) for n, m, *_ in G.exact_cases(h, w))[hname] if hname.startswith("shift") else G.homography(hname, h, w)
    m = G.mask_image(h, w)
    near, sx, sy, _ = R.warp_nearest64(m, Hm)
    nex = R.warp_nearest_excused(sx, sy, h, w)
    assert not ((hname.startswith("shift") or hname == "far") and nex.any())
    t, ws = torch.from_numpy(m).cuda(), ops.mask_bbox_ws()
    boxes = []
    for fill in FILLS:
        warped = Guarded((h, w), fill)
        boxes.append(ops.mask_bbox(t, Hmat=Hm, warped=warped.view, ws=ws).cpu().tolist())
        assert int(ws.view(torch.int32).abs().sum()) == 0                 # the scratch is left zeroed
        got = warped.numpy()
        assert np.isin(got, (0, 255)).all()
        _check_flags(f"mask-nearest {hname} {h}x{w} fill {fill}", near, got, nex, (h, w) in G.THIN)
        assert boxes[-1] == _np_bbox(got)                                  # the box of the mask the launch itself produced
    boxes.append(ops.mask_bbox(t, Hmat=Hm, ws=ws).cpu().tolist())          # without materialising the warped mask
    assert int(ws.view(torch.int32).abs().sum()) == 0
    assert boxes[0] == boxes[1] == boxes[2]
    if not nex.any():
        assert boxes[0] == _np_bbox(near), (boxes[0], _np_bbox(near))


# ---- the input downscale ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", G.RESIZE_FACTORS)
@pytest.mark.parametrize("c", G.CHANNELS)
@pytest.mark.parametrize("h,w", G.RESIZE_SIZES)
def test_resize_against_fp64(h, w, c, factor):
    """ops.resize_by_factor_u8 under the classification rule -- and, beyond it, byte for byte: every factor here gives
    interpolation weights that are multiples of 1/4, so the value is a multiple of 1/16 below 256, exact in fp32, and the byte
    is rint of it, ties half to even, with nothing excused (ties are structural here, up to a quarter of the bytes, which is
    why the rule alone would prove too little).  A size that rounds to 0 rows or columns is an error, not an empty image."""
    img = G.image(h, w, c, seed=1)
    t = torch.from_numpy(img).cuda()
    ho, wo = R.resize_out_shape(h, w, factor)
    assert (ho, wo) == (int(round(h / factor)), int(round(w / factor)))
    if ho == 0 or wo == 0:
        with pytest.raises(_lib.WoftHipError):
            ops.resize_by_factor_u8(t, factor)
        return
    got = ops.resize_by_factor_u8(t, factor)
    assert tuple(got.shape) == (ho, wo) + img.shape[2:]
    got = got.cpu().numpy()
    v = R.resize_linear64(img, factor)
    bad, excused, used = R.classify_bytes(v, got)
    print(f"GEOM resize {h}x{w}x{c} / {factor}: bytes {got.size} on-a-tie {int(excused.sum())} ({100 * G.share(excused):.4f} %) "
          f"used-the-band {int(used.sum())} outside-the-rule {int(bad.sum())}")
    assert not bad.any(), (int(bad.sum()), v[bad][:4], got[bad][:4])
    assert np.array_equal(got, np.rint(v)), int((got != np.rint(v)).sum())
    assert np.array_equal(got, tracker_ref.resize_linear_u8(img, factor))                 # the fp32 oracle: the same bytes
    if factor == 2 and h % 2 == 0 and w % 2 == 0:                          # the 2x2 mean, in integers
        s = img.astype(np.int64).reshape(h // 2, 2, w // 2, 2, -1).sum((1, 3)).reshape(got.shape)
        assert np.array_equal(got, R.rint_div(s, 4))
    for fill in FILLS:                                                     # the C entry point into a guarded output
        g = Guarded(got.shape, fill)
        rc = _lib.load().woft_resize_linear_u8(t.data_ptr(), h, w, c, g.view.data_ptr(), ho, wo, float(factor), float(factor),
                                               _lib.stream_ptr())
        assert rc == 0 and np.array_equal(g.numpy(), got)


# ---- the rectangle copy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("c", G.CHANNELS)
def test_rectangle_copy_into_unaligned_guarded_outputs(c, offset):
    """ops.crop_u8 into an `out` that starts 0 - 3 bytes past a 4-byte boundary (the byte-store path) with guards around it:
    the torch slice, and not one byte more (the tail thread stores fewer than 4 bytes when the count is no multiple of 4)."""
    img = G.image(WIN_H, WIN_W, c, seed=10 + c)
    t = torch.from_numpy(img).cuda()
    rects = dict(WINDOWS, **{"7x5": (3, 4, 7, 5), "1x3": (5, 6, 1, 3), "2x1": (WIN_H - 2, 0, 2, 1)})
    assert (7 * 5 * 3) % 4 != 0
    for name, (y0, x0, rows, cols) in rects.items():
        want = img[y0:y0 + rows, x0:x0 + cols]
        for fill in FILLS:
            g = Guarded(want.shape, fill, offset)
            assert g.view.data_ptr() % 4 == offset
            got = ops.crop_u8(t, (y0, x0, rows, cols), out=g.view)
            assert got.data_ptr() == g.view.data_ptr()
            assert np.array_equal(g.numpy(), want), (c, offset, name, fill)


# ---- argument checks ----------------------------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments():
    """Every argument these entry points reject before launching anything: WOFT_EINVAL, and no byte written."""
    lib = _lib.load()
    img = torch.full((8, 8, 3), 9, dtype=torch.uint8, device="cuda")
    out, valid = torch.full_like(img, 77), torch.full((8, 8), 77, dtype=torch.uint8, device="cuda")
    ws, bbox = torch.zeros(int(lib.woft_mask_bbox_ws_bytes()), dtype=torch.uint8, device="cuda"), torch.full((5,), 77,
                                                                                                              dtype=torch.int32,
                                                                                                              device="cuda")
    hinv = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    pi, po, pv = img.data_ptr(), out.data_ptr(), valid.data_ptr()

    def rejected(fn, base, *subs):
        for sub in subs:
            args = list(base)
            for i, val in sub.items():
                args[i] = val
            assert fn(*args) == EINVAL, (fn.__name__, sub)

    sizes = [{1: 0}, {1: -1}, {2: 0}, {2: -3}, {3: 0}, {3: 5}, {3: -1}]     # h, w, c at the same places in all four image kernels
    # woft_warp_perspective_u8(img, h, w, c, hinv, out, valid, nearest, stream)
    rejected(lib.woft_warp_perspective_u8, [pi, 8, 8, 3, hinv, po, pv, 0, None], {0: None}, {4: None}, {5: None, 6: None},
             {5: None, 7: 1}, *sizes)
    # woft_warp_perspective_window_u8(img, h, w, c, hinv, y0, x0, hw, ww, out, valid, nearest, stream)
    rejected(lib.woft_warp_perspective_window_u8, [pi, 8, 8, 3, hinv, 1, 1, 4, 4, po, pv, 0, None], {0: None}, {4: None},
             {9: None, 10: None}, {9: None, 11: 1}, *sizes, {5: -1}, {6: -1}, {7: 0}, {8: 0}, {7: -2}, {5: 5}, {6: 5}, {7: 8},
             {8: 9}, {5: 8, 7: 1}, {6: 2 ** 31 - 1})
    # woft_crop_u8(img, h, w, c, y0, x0, hw, ww, out, stream)
    rejected(lib.woft_crop_u8, [pi, 8, 8, 3, 1, 1, 4, 4, po, None], {0: None}, {8: None}, *sizes, {4: -1}, {5: -1}, {6: 0},
             {7: 0}, {4: 5}, {5: 5}, {6: 8}, {7: 9}, {4: 2 ** 31 - 1}, {7: 2 ** 31 - 1})
    # woft_resize_linear_u8(img, h, w, c, out, ho, wo, scale_y, scale_x, stream)
    rejected(lib.woft_resize_linear_u8, [pi, 8, 8, 3, po, 4, 4, 2.0, 2.0, None], {0: None}, {4: None}, *sizes, {5: 0}, {6: 0},
             {5: -1}, {6: -4})
    # woft_mask_bbox(mask, h, w, hinv, warped, ws, bbox, stream)
    rejected(lib.woft_mask_bbox, [pv, 8, 8, hinv, po, ws.data_ptr(), bbox.data_ptr(), None], {0: None}, {5: None}, {6: None},
             {1: 0}, {2: 0}, {1: -1}, {2: -1}, {3: None})                  # the last: `warped` without `hinv`
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((valid == 77).all()) and bool((bbox == 77).all()) and not bool(ws.any())
