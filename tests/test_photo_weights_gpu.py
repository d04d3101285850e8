"""woft_photo_weights on the device (csrc/photo_weights.hip) against the numpy restatement of
tests/photo_weights_host.py -- gate maps and support counts byte for byte, soft values against float64 within the float32
restatement's own distance --, and the per-call `weights=` of the photometric refinement: the pinned occlusion cases refined with
the kernel's map against the float64 refinement with the same map, and a per-call map against a constructor's.  Run with -s for
the measured distances."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import photo_host as ph  # noqa: E402
import photo_weights_host as pw  # noqa: E402
from test_photo_gpu import compare_run  # noqa: E402
from woft_amd import _lib, ops, photo  # noqa: E402

RADII, KS = (0, 1, 4), (0, 1, 3, 32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def planes():
    """Per rectangle: the planted planes on the host and on the device."""
    out = {}
    for name, rect in pw.RECTS.items():
        cost, vis = pw.planted_planes(rect)
        out[name] = (rect, cost, vis, dev(cost), dev(vis))
    return out


@pytest.fixture(scope="module")
def targets():
    """Per K: the bit plane on the host (uint32) and on the device (its int32 view)."""
    out = {0: (None, None)}
    for K in KS[1:]:
        bits = pw.pack_bits(pw.target_masks(K))
        out[K] = (bits, dev(bits.view(np.int32)))
    return out


_REFS = {}


def reference(planes, name, mode, radius, dtype):
    """The restatement's map of a case, computed once."""
    key = (name, mode, radius, dtype)
    if key not in _REFS:
        rect, cost, vis = planes[name][:3]
        _REFS[key] = pw.weight_map(cost, vis, pw.TEMPLATE_HW, rect, vis_thr=pw.VIS_THR, mode=mode, radius=radius, dtype=dtype)[0]
    return _REFS[key]


def run(planes, targets, name, K, mode, radius):
    rect, _, _, cost, vis = planes[name]
    wmap = torch.full(pw.TEMPLATE_HW, float("nan"), dtype=torch.float32, device="cuda")
    support = torch.full((max(K, 1),), -7, dtype=torch.int32, device="cuda")
    got = photo.photo_weight_map(cost, vis, pw.TEMPLATE_HW, rect=rect, bits=targets[K][1], n_targets=K, vis_thr=pw.VIS_THR,
                                 mode=mode, erode=radius, out=(wmap, support if K else None))
    assert got[0] is wmap and (got[1] is support if K else got[1] is None)
    return wmap.cpu().numpy(), support.cpu().numpy()[:K]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", sorted(pw.RECTS))
def test_gate_map_and_support_are_the_restatements_bytes(planes, targets, name, radius, K):
    wmap, support = run(planes, targets, name, K, "gate", radius)
    ref = reference(planes, name, "gate", radius, np.float32)
    assert wmap.tobytes() == ref.tobytes()
    if K:
        want = pw.support_counts(ref, targets[K][0], K)
        assert support.dtype == np.int32 and support.tobytes() == want.tobytes(), (support, want)
        assert want[0] > 0 and (K < 32 or want[31] > 0)                # (the counts are not trivially empty; bit 31 is counted)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", sorted(pw.RECTS))
def test_soft_map_against_float64(planes, targets, name, radius, K):
    """The zero pattern and the counts are the float32 restatement's; the values lie within 4 x the float32 restatement's distance
    from the float64 one, with a floor of four fp32 ulps of the value."""
    wmap, support = run(planes, targets, name, K, "soft", radius)
    f32, f64 = (reference(planes, name, "soft", radius, dt) for dt in (np.float32, np.float64))
    assert np.array_equal(wmap > 0, f32 > 0) and np.array_equal(wmap == 0, f32 == 0) and np.array_equal(f64 > 0, f32 > 0)
    if K:
        assert support.tobytes() == pw.support_counts(f32, targets[K][0], K).tobytes()
    yard = float(np.abs(f32.astype(np.float64) - f64).max())
    ulps4 = 4.0 * np.spacing(np.abs(f64).astype(np.float32)).astype(np.float64)
    err = np.abs(wmap.astype(np.float64) - f64)
    print(f"soft {name} radius {radius} K {K}: kernel {err.max():.3e} from float64, float32 restatement {yard:.3e}, "
          f"{np.count_nonzero(wmap)} of {wmap.size} positive")
    assert np.all(err <= np.maximum(4.0 * yard, ulps4)), float(err.max())


def test_planted_zeros_spread_as_stated(planes, targets):
    """The zeros at a template corner, a template edge, past the tile boundaries and at the rectangle's border, read off the
    kernel's own radius-1 map: a corner zero takes the 2 x 2 clipped block, the pixels around (16, 64) -- the first past both tile
    boundaries -- go, and the inner rectangle's border is a zero band."""
    wmap, _ = run(planes, targets, "whole", 0, "gate", 1)
    assert np.all(wmap[:2, :2] == 0) and np.all(wmap[-2:, -2:] == 0)
    assert np.all(wmap[pw.TILE_H - 1:pw.TILE_H + 2, pw.TILE_W - 1:pw.TILE_W + 2] == 0) and np.all(wmap[15:18, 19:22] == 0)
    assert np.all(wmap[19:22, 63:66] == 0) and np.all(wmap[:2, 35:38] == 0)
    assert 0.5 < np.count_nonzero(wmap) / wmap.size < 0.97
    ry, rx, rows, cols = pw.RECTS["inner"]
    wmap, _ = run(planes, targets, "inner", 0, "gate", 1)
    inside = np.zeros(pw.TEMPLATE_HW, bool)
    inside[ry + 1:ry + rows - 1, rx + 1:rx + cols - 1] = True
    assert np.all(wmap[~inside] == 0) and np.count_nonzero(wmap[inside]) > 0.4 * inside.sum()


def test_two_calls_give_equal_bytes(planes, targets):
    for mode in pw.MODES:
        a, b = (run(planes, targets, "whole", 32, mode, 4) for _ in range(2))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_planes_smaller_than_the_template_and_default_rect(planes):
    """rect = None: the planes' own size at origin (0, 0) of a larger template ('crop' padding)."""
    rect, cost, vis, dcost, dvis = planes["inner"]
    got, none = photo.photo_weight_map(dcost.reshape(1, *rect[2:]), dvis.reshape(1, *rect[2:]), pw.TEMPLATE_HW, erode=2)
    want, _ = pw.weight_map(cost, vis, pw.TEMPLATE_HW, (0, 0) + rect[2:], radius=2)
    assert none is None and got.cpu().numpy().tobytes() == want.tobytes()


def test_bad_arguments_return_minus_one(planes, targets):
    lib = _lib.load()
    rect, _, _, cost, vis = planes["inner"]
    bits = targets[3][1]
    wmap = torch.zeros(pw.TEMPLATE_HW, dtype=torch.float32, device="cuda")
    support = torch.zeros(3, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(cost=p(cost), vis=p(vis), rows=rect[2], cols=rect[3], ry=rect[0], rx=rect[1], h=pw.TEMPLATE_HW[0], w=pw.TEMPLATE_HW[1],
             bits=p(bits), K=3, thr=0.5, mode=0, radius=1, out=p(wmap), sup=p(support)):
        return lib.woft_photo_weights(cost, vis, rows, cols, ry, rx, h, w, bits, K, thr, mode, radius, out, sup, ops.stream_ptr())

    assert call() == 0
    for kw in (dict(cost=None), dict(vis=None), dict(out=None), dict(bits=None), dict(sup=None), dict(rows=0), dict(cols=-1),
               dict(ry=17), dict(rx=33), dict(ry=-1), dict(h=0), dict(K=33), dict(K=-1), dict(thr=float("nan")), dict(thr=1.5),
               dict(mode=2), dict(radius=5), dict(radius=-1), dict(out=p(cost)), dict(out=p(bits))):
        assert call(**kw) == -1, kw
    assert call(bits=None, sup=None, K=0) == 0                  # (no targets: neither is needed)
    torch.cuda.synchronize()


# ---- the operator: a per-call weight map ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def occluded():
    """Per seed: the occlusion case and the kernel's map of it (vis = the truth, cost = 0, gate, radius 1), on the device."""
    out = {}
    for seed in ph.SEEDS:
        t, m, f, H_gt, W0, vis = pw.occlusion_case(seed)
        wmap, support = photo.photo_weight_map(torch.zeros(vis.shape), torch.from_numpy(vis), vis.shape,
                                               bits=pw.pack_bits([m > 0]), n_targets=1, mode="gate", erode=1)
        out[seed] = (t, m, f, H_gt, W0, vis, wmap, support)
    return out


@pytest.mark.parametrize("seed", ph.SEEDS)
def test_occlusion_case_refined_with_the_kernels_map(occluded, seed):
    t, m, f, H_gt, W0, vis, wmap, support = occluded[seed]
    want, counts = pw.weight_map(np.zeros_like(vis), vis, vis.shape, bits=pw.pack_bits([m > 0]), n_targets=1, mode="gate", radius=1)
    host_map = wmap.cpu().numpy()
    assert host_map.tobytes() == want.tobytes() and support.cpu().numpy().tobytes() == counts.tobytes()
    kw = dict(iters=6, eps=0.0, gain_bias=True)
    ref = ph.refine(t, m, f, W0, weights=host_map, **kw)
    yard = ph.refine(t, m, f, W0, weights=host_map, dtype=np.float32, **kw)
    got = photo.PhotoTemplate(t, m).refine(f, W0, weights=wmap, **kw)
    worst = compare_run(f"occluded seed {seed}", got, ref, yard, f.shape[:2])
    e_w, e_plain = pw.corner_error(got[0], H_gt), pw.corner_error(photo.refine_homography(t, m, f, W0, **kw)[0], H_gt)
    print(f"occluded seed {seed}: largest kernel distance {worst:.2e} px; corner error weighted {e_w:.3f} px, unweighted {e_plain:.3f} px, "
          f"support {int(support[0])} of {np.count_nonzero(m)}")
    assert e_w <= 0.3 and e_w < 0.5 * e_plain


def _same_info(a, b):
    assert (a.status, a.best, a.n_set) == (b.status, b.best, b.n_set)
    for k in ("H_iter", "gain", "bias", "cost", "n_valid", "step"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


def test_per_call_weights_give_a_constructed_templates_bytes(occluded):
    t, m, f, _, W0, _, wmap, _ = occluded[ph.SEEDS[0]]
    host_map = wmap.cpu().numpy()
    built = photo.PhotoTemplate(t, m, weights=host_map)
    plain = photo.PhotoTemplate(t, m)
    H0, i0 = built.refine(f, W0)
    for weights in (wmap, host_map):                             # (a device tensor, and a numpy map)
        H1, i1 = plain.refine(f, W0, weights=weights)
        assert H0.tobytes() == H1.tobytes()
        _same_info(i0, i1)
        for a, b in zip(built.normal_equations(f, W0), plain.normal_equations(f, W0, weights=weights)):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    H2, i2 = photo.refine_homography(t, m, f, W0, weights=wmap)
    assert H0.tobytes() == H2.tobytes()
    # the call's map replaces the constructor's, and without the argument nothing changes
    other = photo.PhotoTemplate(t, m, weights=np.ones_like(host_map))
    assert other.refine(f, W0, weights=wmap)[0].tobytes() == H0.tobytes()
    Hp, ip = plain.refine(f, W0)
    assert Hp.tobytes() == other.refine(f, W0)[0].tobytes() and Hp.tobytes() != H0.tobytes()
    # a device map is checked for dtype, shape and device only
    for bad in (wmap.double(), wmap[:-1], wmap.cpu().double().numpy()):
        with pytest.raises(ValueError, match="weights"):
            plain.refine(f, W0, weights=bad)
    # a map of zeros: TOO_FEW, no eligible iterate, the input pose back
    Hz, iz = plain.refine(f, W0, weights=torch.zeros_like(wmap))
    assert (iz.status, iz.best) == ("TOO_FEW", -1) and np.array_equal(Hz, W0)


def test_multi_per_call_weights_give_the_single_forms_bytes(occluded):
    t, m, f, _, W0, _, wmap, _ = occluded[ph.SEEDS[1]]
    m2 = np.zeros_like(m)
    m2[8:40, 30:90] = 255
    masks, Hs = [m, m2], np.stack([W0, W0])
    multi = photo.PhotoTemplateMulti(t, masks)
    out, infos = multi.refine(f, Hs, weights=wmap)
    evs = multi.normal_equations(f, Hs, weights=wmap)
    for k, mk in enumerate(masks):
        one = photo.PhotoTemplate(t, mk)
        H1, i1 = one.refine(f, W0, weights=wmap)
        assert out[k].tobytes() == H1.tobytes()
        _same_info(infos[k], i1)
        for a, b in zip(evs[k], one.normal_equations(f, W0, weights=wmap)):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert out[0].tobytes() != multi.refine(f, Hs)[0][0].tobytes()
