"""The float64 restatement of the photometric refinement (tests/photo_host.py) alone: it must meet every
condition tests/test_photo_gpu.py leans on -- the accuracy on the seeded cases, the distance of every warped coordinate from the
validity bounds (a pixel that flips there is a legitimate difference between two correct implementations), the status cases
and the early stop.  Also the argument checks of the new entry points, which work without a device.  Run with -s for the figures."""
import ctypes

import numpy as np
import pytest

import photo_host as ph

MARGIN = 1e-9


@pytest.fixture(scope="module")
def base_runs():
    """{(seed, config): (case, float64 refinement with the defaults, six iterations with eps = 0)}"""
    out = {}
    for seed in ph.SEEDS:
        case = ph.base_case(seed)
        t, m, f, _, W0 = case
        for name, cfg in ph.CONFIGS.items():
            out[seed, name] = (case, ph.refine(t, m, f, W0, **cfg), ph.refine(t, m, f, W0, iters=6, eps=0.0, **cfg))
    return out


def test_accuracy(base_runs):
    """L2 and Huber(6) with gain and bias, three seeds: the final corner error against H_gt is at most a quarter of the initial."""
    for (seed, name), ((t, m, f, H_gt, W0), r, _) in base_runs.items():
        e0, e1 = ph.corner_distance(ph.BOX, W0, H_gt), ph.corner_distance(ph.BOX, r.H, H_gt)
        print(f"seed {seed} {name}: {r.status} best {r.best} of {len(r.cost)}, corner error {e0:.3f} -> {e1:.3f} px, "
              f"cost {r.rms_before:.2f} -> {r.rms_after:.2f} grey levels")
        assert r.best >= 0 and e1 <= 0.25 * e0
        assert r.rms_after <= r.rms_before
        assert r.best == int(np.argmin(r.cost)) and np.array_equal(r.H, r.H_iter[r.best])


def compared_runs(base_runs):
    """Every refinement tests/test_photo_gpu.py compares with the kernels, by name."""
    for (seed, name), (_, r, r6) in base_runs.items():
        yield f"{seed}-{name}", r
        yield f"{seed}-{name}-6", r6
    t, m, f, _, W0 = ph.base_case(ph.SEEDS[0])
    yield "no gain/bias", ph.refine(t, m, f, W0, iters=6, eps=0.0, gain_bias=False)
    yield "stride 2", ph.refine(t, m, f, W0, iters=6, eps=0.0, stride=2)
    t, m, f, _, W0 = ph.partial_case()
    yield "partial", ph.refine(t, m, f, W0)
    t, m, f, _, W0, mv = ph.shrinking_case()
    yield "shrinking", ph.refine(t, m, f, W0, min_valid=mv)


def test_boundary_margins(base_runs):
    """No pixel's u or v is within 1e-9 of a validity bound at any iterate of any compared case."""
    for name, r in compared_runs(base_runs):
        print(f"{name}: smallest distance from a validity bound {r.margin:.3e}")
        assert r.margin > MARGIN, name


def test_float32_yardstick_keeps_the_pixel_set(base_runs):
    """The float32 run of the same steps, the yardstick of the GPU test, has the float64 run's valid pixels at every iterate."""
    for (seed, name), ((t, m, f, _, W0), _, r6) in base_runs.items():
        y = ph.refine(t, m, f, W0, iters=6, eps=0.0, dtype=np.float32, **ph.CONFIGS[name])
        d = [ph.corner_distance(ph.BOX, a, b) for a, b in zip(r6.H_iter, y.H_iter)]
        print(f"seed {seed} {name}: float32 against float64 per iterate " + " ".join(f"{v:.1e}" for v in d))
        assert len(y.cost) == len(r6.cost) == 7 and np.array_equal(y.n_valid, r6.n_valid)
        assert 0 < max(d) < 1e-3


def test_status_cases():
    t, m, f, _, W0 = ph.base_case(ph.SEEDS[0])
    r = ph.refine(np.full_like(t, 77), m, f, W0)
    assert (r.status, r.best, len(r.cost)) == ("SINGULAR", 0, 1)
    one = np.zeros_like(m)
    one[30, 40] = 255
    r = ph.refine(t, one, f, W0)
    assert (r.status, r.best, r.launched) == ("TOO_FEW", -1, False) and np.array_equal(r.H, W0)
    r = ph.refine(t, np.zeros_like(m), f, W0)
    assert (r.status, r.best, r.launched) == ("TOO_FEW", -1, False)
    r = ph.refine(t, m, f, ph.outside_W0())
    assert (r.status, r.best, r.launched, int(r.n_valid[0])) == ("TOO_FEW", -1, True, 0) and np.array_equal(r.H, ph.outside_W0())


def test_partial_mask_changes_n_valid():
    t, m, f, H_gt, W0 = ph.partial_case()
    r = ph.refine(t, m, f, W0)
    print(f"partial: {r.status}, n_valid {r.n_valid.tolist()} of {r.n_set}")
    assert r.status in ("CONVERGED", "MAX_ITERS") and len(set(r.n_valid.tolist())) > 1
    assert r.n_valid.min() >= 0.5 * r.n_set and r.n_valid.max() < r.n_set


def test_falls_below_the_threshold_later():
    t, m, f, _, W0, mv = ph.shrinking_case()
    r = ph.refine(t, m, f, W0, min_valid=mv)
    print(f"shrinking: {r.status}, n_valid {r.n_valid.tolist()}, min_valid {mv:.4f}")
    assert r.status == "TOO_FEW" and len(r.cost) >= 2 and r.best >= 0
    assert r.n_valid[-1] < r.n_valid[0] and np.array_equal(r.H, r.H_iter[r.best])


def test_early_stop_evaluates_one_more_iterate(base_runs):
    seen = 0
    for (seed, name), (_, r, _) in base_runs.items():
        small = np.nonzero(r.step < 1e-3)[0]
        if r.status == "CONVERGED":
            seen += 1
            assert len(small) == 1 and len(r.cost) == small[0] + 2 and np.isnan(r.step[-1])
        else:
            assert r.status == "MAX_ITERS" and len(r.cost) == 11 and (len(small) == 0 or small[0] == 9)
    assert seen >= 1


def test_argument_checks_without_gpu():
    from woft_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.woft_photo_ws_bytes(0, 4, 1) == -1 and lib.woft_photo_ws_bytes(4, 4, 0) == -1
    assert lib.woft_photo_ws_bytes(57, 40, 1) == (2 * 68 + 18) * 8          # (2280 candidates: two chunks of 2048)
    box = (ctypes.c_int32 * 4)(1, 1, 3, 3)
    W = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    p = ctypes.c_void_p(64)                                                  # (never dereferenced: every call is rejected)
    ev = lambda *a: lib.woft_photo_eval(*a)
    rf = lambda *a: lib.woft_photo_refine(*a)
    assert ev(None, 0, p, 5, 7, None, p, 0, 9, 9, box, 1, W, 1.0, 0.0, 1, -1.0, p, p, None) == -1
    assert ev(p, 0, p, 5, 7, None, p, 0, 9, 9, box, 0, W, 1.0, 0.0, 1, -1.0, p, p, None) == -1          # stride
    assert ev(p, 0, p, 5, 7, None, p, 0, 9, 9, box, 1, W, 1.0, 0.0, 1, 0.0, p, p, None) == -1           # huber_k = 0
    assert ev(p, 0, p, 5, 7, None, p, 0, 9, 9, box, 1, W, 1.0, 0.0, 1, -1.0, p, None, None) == -1       # out
    assert ev(p, 0, p, 2, 7, None, p, 0, 9, 9, box, 1, W, 1.0, 0.0, 1, -1.0, p, p, None) == -1          # h < 3
    bad = (ctypes.c_int32 * 4)(1, 1, 7, 3)
    assert ev(p, 0, p, 5, 7, None, p, 0, 9, 9, bad, 1, W, 1.0, 0.0, 1, -1.0, p, p, None) == -1          # box leaves the template
    assert rf(p, 0, p, 5, 7, None, p, 0, 9, 9, box, 1, W, 65, 1, -1.0, 10, 1e-3, p, p, None) == -1      # iters
    assert rf(p, 0, p, 5, 7, None, p, 0, 9, 9, box, 1, W, 3, 1, -1.0, 10, -1.0, p, p, None) == -1       # eps
    assert rf(p, 0, p, 5, 7, None, p, 0, 9, 9, box, 1, W, 3, 1, -1.0, 10, 1e-3, None, p, None) == -1    # ws
    assert rf(p, 0, p, 5, 7, None, p, 0, 9, 9, box, 1, W, 3, 1, -1.0, 10, 1e-3, p, None, None) == -1    # result
    Wn = (ctypes.c_double * 9)(1, 0, 0, 0, float("nan"), 0, 0, 0, 1)
    assert rf(p, 0, p, 5, 7, None, p, 0, 9, 9, box, 1, Wn, 3, 1, -1.0, 10, 1e-3, p, p, None) == -1


def test_python_option_checks():
    from woft_amd import photo
    for kw in (dict(iters=-1), dict(iters=2.5), dict(iters=65), dict(huber_k=0.0), dict(huber_k=float("nan")), dict(min_valid=1.5),
               dict(eps=-1.0), dict(eps=float("inf"))):
        with pytest.raises(ValueError):
            photo.check_options(**{**photo.DEFAULTS, **kw})
    assert photo.check_options(**photo.DEFAULTS) == (10, True, None, 0.5, 1e-3)
    import woft_amd
    assert woft_amd.PhotoTemplate is photo.PhotoTemplate and woft_amd.refine_homography is photo.refine_homography
