"""The visibility weight map of the photometric refinement without a device: the numpy restatement's own
properties (tests/photo_weights_host.py), the pinned occlusion cases on the float64 restatement of the refinement
(tests/photo_host.py), every argument woft_photo_weights rejects -- rejected before the device is touched -- and the Python checks
that need no device."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import photo_host as ph
import photo_weights_host as pw


# ---- the restatement's own properties --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(pw.RECTS))
def case(request):
    rect = pw.RECTS[request.param]
    cost, vis = pw.planted_planes(rect)
    return request.param, rect, cost, vis


def test_gate_values_and_radius_zero_is_raw(case):
    _, rect, cost, vis = case
    for mode in pw.MODES:
        raw = pw.raw_map(cost, vis, pw.TEMPLATE_HW, rect, pw.VIS_THR, mode)
        m0, _ = pw.weight_map(cost, vis, pw.TEMPLATE_HW, rect, vis_thr=pw.VIS_THR, mode=mode, radius=0)
        assert m0.dtype == np.float32 and np.array_equal(m0.view(np.uint32), raw.view(np.uint32))
        assert np.all(np.isfinite(raw)) and np.all(raw >= 0)
    gate = pw.raw_map(cost, vis, pw.TEMPLATE_HW, rect, pw.VIS_THR, "gate")
    assert set(np.unique(gate)) == {0.0, 1.0}
    soft = pw.raw_map(cost, vis, pw.TEMPLATE_HW, rect, pw.VIS_THR, "soft")
    assert np.array_equal(soft > 0, gate > 0)                  # (costs in [0, 3): no product under- or overflows)


def test_planted_values(case):
    _, rect, cost, vis = case
    ry, rx, rows, cols = rect
    raw = pw.raw_map(cost, vis, pw.TEMPLATE_HW, rect, pw.VIS_THR, "gate")[ry:ry + rows, rx:rx + cols]
    at = lambda cond: tuple(np.argwhere(cond)[0])
    assert raw[at(np.isposinf(cost))] == 0 and raw[at(np.isneginf(cost))] == 0 and raw[at(np.isnan(cost))] == 0
    assert raw[at(np.isnan(vis))] == 0
    assert raw[at(vis == np.float32(pw.VIS_THR))] == 1          # the threshold itself passes
    assert raw[at(vis == np.nextafter(np.float32(pw.VIS_THR), np.float32(0)))] == 0


def test_erosion_is_monotone_in_the_radius(case):
    _, rect, cost, vis = case
    for mode in pw.MODES:
        maps = [pw.weight_map(cost, vis, pw.TEMPLATE_HW, rect, vis_thr=pw.VIS_THR, mode=mode, radius=r)[0] for r in range(5)]
        for a, b in zip(maps, maps[1:]):
            assert np.all(b <= a) and np.any(b < a)


def test_template_border_is_clipped_and_rectangle_border_is_a_zero_band():
    h, w = pw.TEMPLATE_HW
    ones = lambda rect: (np.zeros(rect[2:], np.float32), np.ones(rect[2:], np.float32))
    for r in range(5):
        # every pixel passes and the rectangle is the template: neighbours outside the template are ignored, nothing is eroded
        m, _ = pw.weight_map(*ones(pw.RECTS["whole"]), pw.TEMPLATE_HW, pw.RECTS["whole"], radius=r)
        assert np.all(m == 1)
        # the inner rectangle: template pixels outside it count as 0, so a band of r pixels inside its border goes
        ry, rx, rows, cols = pw.RECTS["inner"]
        m, _ = pw.weight_map(*ones(pw.RECTS["inner"]), pw.TEMPLATE_HW, pw.RECTS["inner"], radius=r)
        want = np.zeros((h, w), np.float32)
        want[ry + r:ry + rows - r, rx + r:rx + cols - r] = 1
        assert np.array_equal(m, want)
    # a rectangle that touches the template's corner: clipped on those two sides, a zero band on the other two
    rect = (0, 0, 10, 12)
    m, _ = pw.weight_map(*ones(rect), pw.TEMPLATE_HW, rect, radius=2)
    want = np.zeros((h, w), np.float32)
    want[:8, :10] = 1
    assert np.array_equal(m, want)
    # one failing pixel in a template corner takes its (r + 1)^2 clipped neighbourhood with it
    cost, vis = ones(pw.RECTS["whole"])
    vis[0, 0] = 0
    m, _ = pw.weight_map(cost, vis, pw.TEMPLATE_HW, pw.RECTS["whole"], radius=3)
    assert np.count_nonzero(m == 0) == 16 and np.all(m[:4, :4] == 0)


@pytest.mark.parametrize("mode, radius", [("gate", 0), ("gate", 1), ("soft", 1), ("gate", 4)])
def test_map_and_support_equal_a_brute_force_count(case, mode, radius):
    _, rect, cost, vis = case
    K = 3
    bits = pw.pack_bits(pw.target_masks(K))
    m, s = pw.weight_map(cost, vis, pw.TEMPLATE_HW, rect, bits, K, pw.VIS_THR, mode, radius)
    mb, sb = pw.brute_force(cost, vis, pw.TEMPLATE_HW, rect, bits, K, pw.VIS_THR, mode, radius)
    assert np.array_equal(m.view(np.uint32), mb.view(np.uint32)) and np.array_equal(s, sb) and s.dtype == np.int32
    assert s[0] > 0                                            # (a mask outside the rectangle counts nothing: also a case)


def test_support_uses_bit_31():
    rect = pw.RECTS["whole"]
    cost, vis = pw.planted_planes(rect)
    masks = pw.target_masks(32)
    bits = pw.pack_bits(masks)
    assert bits.max() >= 1 << 31
    m, s = pw.weight_map(cost, vis, pw.TEMPLATE_HW, rect, bits, 32, pw.VIS_THR, "gate", 1)
    assert [int(v) for v in s] == [int(np.count_nonzero(mk & (m > 0))) for mk in masks] and s[31] > 1000


# ---- the occlusion cases, pinned ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def occluded():
    """Per seed: the case, its weight map (truth as vis, cost 0, gate, radius 1) and the float64 refinements without and with it."""
    out = {}
    for seed in ph.SEEDS:
        template, mask, frame, H_gt, W0, vis = pw.occlusion_case(seed)
        wmap, _ = pw.weight_map(np.zeros_like(vis), vis, mask.shape, mode="gate", radius=1)
        plain = ph.refine(template, mask, frame, W0, iters=10, gain_bias=True)
        weighted = ph.refine(template, mask, frame, W0, iters=10, gain_bias=True, weights=wmap)
        out[seed] = (template, mask, frame, H_gt, W0, vis, wmap, plain, weighted)
    return out


@pytest.mark.parametrize("seed", ph.SEEDS)
def test_occlusion_case_pinned(occluded, seed):
    template, mask, frame, H_gt, W0, vis, wmap, plain, weighted = occluded[seed]
    covered = np.count_nonzero((vis == 0) & (mask > 0)) / np.count_nonzero(mask)
    e0, e_plain, e_w = pw.corner_error(W0, H_gt), pw.corner_error(plain.H, H_gt), pw.corner_error(weighted.H, H_gt)
    print(f"seed {seed}: occluder over {covered:.1%} of the mask, start {e0:.3f} px, unweighted L2 {e_plain:.3f} px, "
          f"weight map radius 1 {e_w:.3f} px ({weighted.status})")
    assert 0.2 < covered < 0.45 and 1.6 < e0 < 1.8
    assert e_w <= 0.3
    assert e_w < 0.5 * e_plain
    assert e_plain > 0.7


def test_a_map_of_zeros_is_too_few(occluded):
    template, mask, frame, H_gt, W0 = occluded[ph.SEEDS[0]][:5]
    r = ph.refine(template, mask, frame, W0, weights=np.zeros(mask.shape, np.float32))
    assert r.status == "TOO_FEW" and r.best == -1 and np.array_equal(r.H, W0)


# ---- the entry point's argument checks -------------------------------------------------------------------------------------------------
def _lib():
    from woft_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_argument_checks_without_gpu():
    lib = _lib()
    a, b, c, d, e = (ctypes.c_void_p(4096 * (1 + 1000 * k)) for k in range(5))      # (never dereferenced: every call is rejected)

    def call(cost=a, vis=b, rows=24, cols=40, ry=5, rx=9, h=40, w=72, bits=c, K=3, thr=0.5, mode=0, radius=1, out=d, support=e):
        return lib.woft_photo_weights(cost, vis, rows, cols, ry, rx, h, w, bits, K, thr, mode, radius, out, support, None)

    bad = [dict(cost=None), dict(vis=None), dict(out=None), dict(bits=None), dict(support=None), dict(rows=0), dict(cols=0),
           dict(h=0), dict(w=-1), dict(h=1 << 16, w=1 << 15), dict(ry=-1), dict(rx=-1), dict(ry=17), dict(rx=33), dict(rows=41, ry=0),
           dict(K=-1), dict(K=33), dict(thr=float("nan")), dict(thr=-0.1), dict(thr=1.5), dict(mode=2), dict(mode=-1),
           dict(radius=-1), dict(radius=5),
           dict(out=a), dict(out=b), dict(out=c), dict(support=d), dict(out=ctypes.c_void_p(4096 + 24 * 40 * 4 - 4))]
    for kw in bad:
        assert call(**kw) == -1, kw
    from woft_amd import _lib as L, ops
    assert "woft_photo_weights" in L.EXPORTS and ops.PHOTO_WEIGHTS_MAX_RADIUS == pw.MAX_RADIUS and ops.PHOTO_WEIGHT_MODES == pw.MODES
    header = (Path(__file__).resolve().parent.parent / "include" / "woft_hip.h").read_text()
    assert "int woft_photo_weights(" in header and "#define WOFT_PHOTO_WEIGHTS_MAX_RADIUS 4" in header


def test_python_checks_without_gpu():
    import torch
    import woft_amd
    from woft_amd import photo
    assert woft_amd.photo_weight_map is photo.photo_weight_map
    z = torch.zeros(4, 6)
    for kw in (dict(mode="hard"), dict(erode=5), dict(erode=-1), dict(erode=1.0), dict(erode=True), dict(vis_thr=1.5),
               dict(vis_thr=float("nan")), dict(n_targets=33), dict(n_targets=-1), dict(n_targets=1), dict(rect=(0, 0, 4)),
               dict(rect=(1, 0, 4, 6)), dict(rect=(0, 0, 4, 5)), dict(template_hw=(3, 6))):
        with pytest.raises(ValueError):
            photo.photo_weight_map(z, z, **{"template_hw": (4, 6), **kw})
    with pytest.raises(TypeError):
        photo.photo_weight_map(np.zeros((4, 6), np.float32), z, (4, 6))
    # a per-call numpy map is checked as the constructor checks its own
    for wt in (np.zeros((4, 6), np.float64), np.zeros((4, 5), np.float32), np.full((4, 6), -1.0, np.float32),
               np.full((4, 6), np.nan, np.float32)):
        with pytest.raises(ValueError, match="weights"):
            photo._call_weights(None, wt, 4, 6, "cpu")
    assert photo._call_weights("own", None, 4, 6, "cpu") == "own"
