"""The search-window tracker's host side (woft_amd/window.py, the shim, the config, argument checks of the window kernels' entry
points): no GPU.  Boxes are checked against the ones the REFERENCE's own WOFTWindow used in the recorded runs
(tests/golden/tracker_window_runs.npz, tools/gen_window_golden.py) and against hand cases."""
import ctypes

import numpy as np
import pytest

from woft_amd import window
from woft_amd.window import Box, H_undo_crop, search_box


@pytest.fixture(scope="module")
def runs(golden_dir):
    return np.load(golden_dir / "tracker_window_runs.npz")


def test_box_corners_are_inclusive_and_crop_is_exclusive():
    b = Box(10, 20, 30, 40)
    assert (b.br_x, b.br_y) == (39, 59)
    assert Box.from_xyxy(10, 20, 39, 59) == b
    img = np.arange(100 * 120 * 3).reshape(100, 120, 3)
    crop = b.crop_image(img)
    assert crop.shape == (39, 29, 3)                      # a box of width w crops w - 1 columns
    assert np.array_equal(crop, img[20:59, 10:39])
    assert b.crop_rect() == (20, 10, 39, 29)
    assert Box.frame(120, 100).crop_image(img).shape == (99, 119, 3)        # the whole-frame box drops the last row and column


def test_from_mask_and_the_all_zero_mask():
    m = np.zeros((50, 70), np.uint8)
    assert Box.from_mask(m) == Box(0, 0, 1, 1)
    m[7, 9] = 255
    assert Box.from_mask(m) == Box(9, 7, 1, 1)
    m[20:31, 3:66] = 1
    assert Box.from_mask(m) == Box(3, 7, 63, 24)
    assert Box.from_mask(m > 0) == Box(3, 7, 63, 24)
    assert Box.from_extent(7, 30, 3, 65) == Box(3, 7, 63, 24)
    assert Box.from_extent(5, 6, 7, 8, any_set=False) == Box(0, 0, 1, 1)


def test_margins_truncate_the_product():
    b = Box(100, 100, 10, 7)
    g = b.with_margins(0.25)                               # int(2.5) = 2, int(1.75) = 1
    assert (g.tl_x, g.tl_y, g.br_x, g.br_y) == (98, 99, 111, 107)
    assert g == Box(98, 99, 14, 9)
    assert b.with_margins(0.09) == b                       # int(0.9) = 0 on both axes


def test_min_size_grows_both_axes_by_the_larger_fraction():
    b = Box(100, 80, 120, 96)
    g = b.with_margins_min_size(160)
    need = max(20 / 120, 32 / 96)
    assert g == b.with_margins(need)
    assert g.h >= 159 and g.w >= 160                       # (the truncation may leave one pixel short: the reference's arithmetic)
    assert Box(0, 0, 200, 170).with_margins_min_size(160) == Box(0, 0, 200, 170)
    assert Box(50, 50, 200, 100).with_margins_min_size(160, 100) == Box(50, 50, 200, 100)


def test_intersection():
    assert Box(-10, -5, 50, 50).intersection(Box.frame(30, 100)) == Box(0, 0, 30, 45)
    assert Box(5, 6, 10, 10).intersection(Box.frame(320, 256)) == Box(5, 6, 10, 10)


def test_undo_crop_composed_with_its_inverse_is_the_identity():
    rs = np.random.RandomState(0)
    b = Box(37, 21, 100, 90)
    H = np.eye(3) + 0.01 * rs.randn(3, 3)
    H /= H[2, 2]
    F = H_undo_crop(b, H)
    back = H_undo_crop(Box(-37, -21, 100, 90), F)          # cropping the other way round undoes it
    assert np.allclose(back / back[2, 2], H, atol=1e-12)
    assert np.allclose(H_undo_crop(b, np.eye(3)), np.eye(3))
    p = np.array([50.0, 60.0, 1.0])                        # a frame point, mapped in window coordinates and brought back
    q = H @ (p - [37, 21, 0])
    q = q / q[2] + [37, 21, 0]
    r = F @ p
    assert np.allclose(r / r[2], q, atol=1e-9)


def test_search_boxes_equal_the_reference_runs(runs):
    """init's box and every lost frame's box of every recorded run, from the same inputs: integers, equal."""
    n_local = 0
    for name in runs["runs"]:
        mask = runs[f"{name}_mask"]
        k = int(runs[f"{name}_downscale"]) or 1
        if k > 1:                                          # (0 / 255 rectangle with even edges: every second pixel is the resize)
            mask = mask[::k, ::k]
        Hh, Ww = mask.shape
        margin = float(runs[f"{name}_margin"]) or None
        box = search_box(Box.from_mask(mask > 0), margin, Ww, Hh)
        assert box.as_xywh() == tuple(runs[f"{name}_search_box"]), name
        assert box == search_box(Box.from_mask(mask > 0), margin, Ww, Hh, clip=False)     # no golden run depends on the clip
        assert box.inside(Ww, Hh)
        # local boxes: the carried mask is the template mask warped (nearest) by the inverse of the previous pose
        Hs = runs[f"{name}_H"]
        S, Sinv = np.diag([1.0 / k, 1.0 / k, 1.0]), np.diag([float(k), float(k), 1.0])
        for row in runs[f"{name}_local_boxes"]:
            i = int(row[0])
            prev = np.eye(3) if i == 0 else S @ Hs[i - 1] @ Sinv        # (track() returns the pose at input scale)
            P = np.linalg.inv(np.linalg.inv(prev))                       # nearest-neighbour warp by inv(prev): dst(x) = src(prev x)
            ys, xs = np.mgrid[0:Hh, 0:Ww].astype(np.float64)
            d = P[2, 0] * xs + P[2, 1] * ys + P[2, 2]
            sx, sy = np.rint((P[0, 0] * xs + P[0, 1] * ys + P[0, 2]) / d), np.rint((P[1, 0] * xs + P[1, 1] * ys + P[1, 2]) / d)
            ok = (sx >= 0) & (sx < Ww) & (sy >= 0) & (sy < Hh)
            carried = np.zeros((Hh, Ww), bool)
            carried[ok] = mask[sy[ok].astype(int), sx[ok].astype(int)] > 0
            box = search_box(Box.from_mask(carried), margin, Ww, Hh)
            assert box.as_xywh() == tuple(row[1:]), (name, i, box, row)
            assert box == search_box(Box.from_mask(carried), margin, Ww, Hh, clip=False) and box.inside(Ww, Hh)
            n_local += 1
    assert n_local >= 2


def test_box_pushed_past_the_frame_edge_is_clipped():
    """Deviation from the reference: a small mask in a corner -- the minimum-size step pushes the box to negative coordinates, where
    the reference slices with a negative index; here the box is cut to the frame."""
    m = np.zeros((256, 320), np.uint8)
    m[4:44, 6:56] = 255
    ref_box = search_box(Box.from_mask(m), 0.25, 320, 256, clip=False)
    assert ref_box.tl_x < 0 and ref_box.tl_y < 0 and not ref_box.inside(320, 256)
    box = search_box(Box.from_mask(m), 0.25, 320, 256)
    assert box.inside(320, 256) and (box.tl_x, box.tl_y) == (0, 0)
    assert (box.br_x, box.br_y) == (ref_box.br_x, ref_box.br_y)
    y0, x0, rows, cols = box.crop_rect()
    assert y0 >= 0 and x0 >= 0 and y0 + rows <= 256 and x0 + cols <= 320 and rows > 40 and cols > 50
    assert search_box(Box.from_mask(m), None, 320, 256) == Box.frame(320, 256)
    assert search_box(Box.from_mask(m), 0, 320, 256) == Box.frame(320, 256)


def test_shim_path_and_config():
    from pathlib import Path
    from pytracking.tracker.WOFT_window import WOFTWindow, H_undo_crop as shim_undo
    from pytracking.tracker.YAOF_tracker_single_control import YAOFTrackerSingleControl
    from pytracking.utils.config import load_config
    import woft_amd.tracker
    assert WOFTWindow is woft_amd.tracker.WOFTWindow and issubclass(WOFTWindow, YAOFTrackerSingleControl)
    assert shim_undo is window.H_undo_crop
    for attr in ("init", "track", "set_fast_meta"):
        assert callable(getattr(WOFTWindow, attr))
    root = Path(__file__).resolve().parent.parent
    conf = load_config(root / "pytracking" / "configs" / "WOFT_window.py")
    base = load_config(root / "pytracking" / "configs" / "WOFT.py")
    assert conf.tracker_class is WOFTWindow and conf.search_window_margin == 0.25
    assert base.tracker_class is YAOFTrackerSingleControl and not base.search_window_margin
    assert conf.no_prewarp_after_N == base.no_prewarp_after_N
    # the probe reaches the same solver decision for both configs
    from woft_amd.probe import solver_spec
    from woft_amd.tracker import make_forward_compatible
    a = solver_spec(conf.H_estimator, make_forward_compatible(conf.subsampler_fn), conf.redet_success_fn, device="cpu")
    b = solver_spec(base.H_estimator, make_forward_compatible(base.subsampler_fn), base.redet_success_fn, device="cpu")
    assert a[0] is not None and a == b


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_window_entry_points_reject_bad_arguments_without_a_device(lib):
    """-1 before any launch: NULL pointers, empty rectangles, rectangles that leave the frame.  (The pointers are host buffers that
    no accepted call ever sees: every call below is rejected.)"""
    buf = ctypes.create_string_buffer(64 * 64 * 3)
    out = ctypes.create_string_buffer(64 * 64 * 3)
    p, o = ctypes.addressof(buf), ctypes.addressof(out)
    hinv = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    warp, crop, bbox = lib.woft_warp_perspective_window_u8, lib.woft_crop_u8, lib.woft_mask_bbox
    bad_rects = [(0, 0, 0, 10), (0, 0, 10, 0), (-1, 0, 10, 10), (0, -1, 10, 10), (60, 0, 5, 10), (0, 60, 10, 5), (0, 0, 65, 64),
                 (0, 0, 64, 65), (2 ** 31 - 1, 0, 2, 2)]
    for y0, x0, rows, cols in bad_rects:
        assert warp(p, 64, 64, 3, hinv, y0, x0, rows, cols, o, o, 0, None) == -1, (y0, x0, rows, cols)
        assert crop(p, 64, 64, 3, y0, x0, rows, cols, o, None) == -1, (y0, x0, rows, cols)
    assert warp(None, 64, 64, 3, hinv, 0, 0, 8, 8, o, o, 0, None) == -1
    assert warp(p, 64, 64, 3, None, 0, 0, 8, 8, o, o, 0, None) == -1
    assert warp(p, 64, 64, 3, hinv, 0, 0, 8, 8, None, None, 0, None) == -1
    assert warp(p, 64, 64, 3, hinv, 0, 0, 8, 8, None, o, 1, None) == -1          # nearest needs an image output
    assert warp(p, 64, 64, 5, hinv, 0, 0, 8, 8, o, o, 0, None) == -1
    assert warp(p, 0, 64, 3, hinv, 0, 0, 8, 8, o, o, 0, None) == -1
    assert crop(None, 64, 64, 3, 0, 0, 8, 8, o, None) == -1
    assert crop(p, 64, 64, 3, 0, 0, 8, 8, None, None) == -1
    assert crop(p, 64, 64, 0, 0, 0, 8, 8, o, None) == -1
    assert lib.woft_mask_bbox_ws_bytes() >= 20
    assert bbox(None, 64, 64, None, None, o, o, None) == -1
    assert bbox(p, 64, 64, None, None, None, o, None) == -1
    assert bbox(p, 64, 64, None, None, o, None, None) == -1
    assert bbox(p, 0, 64, None, None, o, o, None) == -1
    assert bbox(p, 64, -1, None, None, o, o, None) == -1
    assert bbox(p, 64, 64, None, o, o, o, None) == -1                            # a warped output without a homography
