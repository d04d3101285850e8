"""The RANSAC similarity estimator (find_homography_TRS) without a GPU: the semantics of csrc/trs.hip as the host restatement
(tests/trs_host.py) states them -- the adaptive stop, the inlier mask and the closed-form refit on a known similarity --, the C ABI
entries reject bad arguments before touching the device, header and exports agree, the probe recognises the preset and a
reference-form config (tests/configs/reference_forms_trs.py) and refuses what it cannot run, and the shim config loads."""
import ctypes
import re
import sys
import types
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import trs_host as th  # noqa: E402

W_IMG, H_IMG = 640, 480
_ANG = np.deg2rad(3.0)
S_TRUE = np.array([[1.05 * np.cos(_ANG), -1.05 * np.sin(_ANG), 12.0], [1.05 * np.sin(_ANG), 1.05 * np.cos(_ANG), -7.0],
                   [0.0, 0.0, 1.0]])
CORNERS = np.array([[0, 0], [W_IMG, 0], [W_IMG, H_IMG], [0, H_IMG]], np.float64)


def _proj(H, p):
    q = np.c_[p, np.ones(len(p))] @ np.asarray(H, np.float64).T
    return q[:, :2] / q[:, 2:]


def _corner_err(Ha, Hb):
    return float(np.linalg.norm(_proj(Ha, CORNERS) - _proj(Hb, CORNERS), axis=1).max())


def make_points(n, sigma, outliers, seed, H=S_TRUE):
    """Correspondences a -> S a (+ N(0, sigma) px); a fraction `outliers` of them moved 20 to 60 px away in a random direction.
    -> (pa, pb) float32 (n, 2), inlier ground truth (n,) bool."""
    rng = np.random.default_rng(seed)
    a = rng.random((n, 2)) * [W_IMG, H_IMG]
    b = _proj(H, a) + rng.normal(0.0, sigma, (n, 2)) * (sigma > 0)
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:int(round(outliers * n))]] = True
    ang = rng.random(out.sum()) * 2 * np.pi
    r = 20.0 + 40.0 * rng.random(out.sum())
    b[out] += np.c_[np.cos(ang), np.sin(ang)] * r[:, None]
    return a.astype(np.float32), b.astype(np.float32), ~out


# ---- the semantics, on the host restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [500, 4096])
@pytest.mark.parametrize("outliers,stop", [(0.0, 1), (0.3, 10), (0.6, 40)])
def test_noise_free_stop_mask_and_refit(n, outliers, stop):
    # the stop: round(ln 0.001 / ln(1 - w^2)) for an inlier fraction w -- 1 (w = 1: niters -> 0), 10 (w = 0.7), 40 (w = 0.4)
    for seed in (0, 1, 12345):
        pa, pb, gt = make_points(n, 0.0, outliers, 100 * n + seed)
        r = th.fit_host(pa, pb, max_iters=1000, thr=3.0, conf=0.999, seed=seed)
        assert r["status"] == 0 and r["iterations"] == stop, (seed, r["iterations"])
        assert np.array_equal(r["mask"], gt) and r["n_inliers"] == int(gt.sum()), seed
        assert np.array_equal(r["H"][2], [0.0, 0.0, 1.0])
        assert _corner_err(r["H"], S_TRUE) < 1e-4, (seed, _corner_err(r["H"], S_TRUE))       # (fp32 storage of the inputs)


@pytest.mark.parametrize("outliers", [0.0, 0.3, 0.6])
def test_noisy_inliers_no_outlier_enters_the_mask(outliers):
    for seed in (0, 1, 12345):
        pa, pb, gt = make_points(500, 0.5, outliers, 100 * 500 + seed)
        r = th.fit_host(pa, pb, max_iters=1000, thr=3.0, conf=0.999, seed=seed)
        assert r["status"] == 0 and not np.any(r["mask"] & ~gt), seed
        assert _corner_err(r["H"], S_TRUE) < 0.5, (seed, _corner_err(r["H"], S_TRUE))


def test_small_and_degenerate_sets():
    a = np.array([[10, 20], [300, 40]], np.float32)
    b = _proj(S_TRUE, a).astype(np.float32)
    r = th.fit_host(a, b)
    assert (r["status"], r["iterations"], r["best_k"], r["n_inliers"]) == (0, 0, 0, 2) and r["mask"].all()
    assert np.abs(_proj(r["H"], a) - b).max() < 1e-4
    same = np.full((16, 2), 7.0, np.float32)                    # every A point identical: every model degenerate
    r = th.fit_host(same, same + 1, max_iters=50)
    assert r["status"] == 2 and r["best_k"] == -1 and np.isnan(r["H"]).all() and not r["mask"].any()
    assert th.update_num_iters(0.999, 0.3, 1000) == 10 and th.update_num_iters(0.999, 0.6, 1000) == 40
    assert th.update_num_iters(0.999, 0.0, 1000) == 0 and th.update_num_iters(0.999, 1.0, 1000) == 1000


# ---- C ABI, header, library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_trs_abi_rejects_bad_arguments(lib):
    buf = (ctypes.c_float * 64)()
    st = (ctypes.c_int32 * 4)()
    p = ctypes.addressof(buf)
    s = ctypes.addressof(st)
    ok = dict(pa=p, pb=p, n_max=8, count=None, max_iters=100, thr=3.0, conf=0.999, seed=0, refine=1, ws=p, Hout=p, status=s,
              info=None, mask=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.woft_trs(a["pa"], a["pb"], a["n_max"], a["count"], a["max_iters"], a["thr"], a["conf"], a["seed"],
                            a["refine"], a["ws"], a["Hout"], a["status"], a["info"], a["mask"], a["stream"])
    for bad in (dict(pa=None), dict(pb=None), dict(ws=None), dict(Hout=None), dict(status=None), dict(n_max=-1),
                dict(max_iters=0), dict(max_iters=-5), dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")),
                dict(conf=-0.01), dict(conf=1.01), dict(conf=float("nan"))):
        assert call(**bad) == -1, bad
    assert lib.woft_trs_ws_bytes(-1, 10) == -1 and lib.woft_trs_ws_bytes(10, 0) == -1
    assert lib.woft_trs_ws_bytes(500, 10000) >= 4 * 10000            # (the workspace begins with the per-hypothesis counts)


def test_trs_header_and_exports(lib):
    from woft_amd import _lib
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    assert {"woft_trs", "woft_trs_ws_bytes"} <= declared
    assert {"woft_trs", "woft_trs_ws_bytes"} <= set(_lib.EXPORTS)
    assert lib.woft_trs is not None and lib.woft_trs_ws_bytes is not None
    assert lib.woft_abi_version() == 400                             # (additions only: the version stays)


# ---- probe, preset, shim -------------------------------------------------------------------------------------------------
def _reference_form_config():
    path = ROOT / "tests" / "configs" / "reference_forms_trs.py"
    m = types.ModuleType("tracker_config")
    m.__file__ = str(path)
    exec(compile(path.read_text(), str(path), "exec"), m.__dict__)
    return m.get_config()


def test_trs_preset_is_tagged_and_probe_agrees():
    from woft_amd import presets, probe
    est = presets.estimator_trs()
    assert est.woft_spec == ("trs", 10000, 3.0, 0.999)
    assert probe.probe_estimator(est) == ("trs", 10000, 3.0, 0.999, False)
    est = presets.estimator_trs(max_iters=2000, thr=2.5, conf=0.99)
    assert probe.probe_estimator(est) == ("trs", 2000, 2.5, 0.99, False)


def test_probe_recognises_the_reference_form_trs_config():
    from woft_amd import probe
    from woft_amd.tracker import make_forward_compatible
    sys.dont_write_bytecode = True
    conf = _reference_form_config()
    assert probe.probe_estimator(conf.H_estimator) == ("trs", 10000, 3.0, 0.999, False)
    spec, how = probe.solver_spec(conf.H_estimator, make_forward_compatible(conf.subsampler_fn), conf.redet_success_fn)
    assert spec is not None and how.count("probed") == 3, how
    assert spec["trs"] == dict(max_iters=10000, thr=3.0, conf=0.999) and spec["weighted"] is False and "ransac" not in spec
    assert (spec["thr"], spec["min_frac"], spec["n_draw"], spec["const_verdict"]) == (5.0, 0.2, 500, None)


def test_probe_rejects_trs_forms_it_cannot_run():
    from woft_amd import probe
    from woft_amd.homography import find_homography_TRS as trs
    assert probe.probe_estimator(lambda a, b, weights=None: trs(a, b)) == ("trs", 10000, 3.0, 0.999, False)
    assert probe.probe_estimator(lambda a, b, weights=None: trs(a, b) * 1.0) is None                   # post-processed result
    assert probe.probe_estimator(lambda a, b, weights=None: trs(a, b, thr=3.0 + a.shape[1] / 1000)) is None   # thr varies per call
    assert probe.probe_estimator(lambda a, b, weights=None: trs(a, b, max_iters=a.shape[1] * 10)) is None
    assert probe.probe_estimator(lambda a, b, weights=None: trs(a, b, thr=-1)) is None
    assert probe.probe_estimator(lambda a, b, weights=None: trs(a * 2, b)) is None
    spec, how = probe.solver_spec(lambda a, b, weights=None: trs(a, b) * 1.0, None, lambda *a: True)
    assert spec is None and "estimator: callable" in how                                               # keeps the callable back end


def test_trs_shim_config_loads():
    from pytracking.utils.config import load_config
    from pytracking.utils.least_squares_H import find_homography_TRS
    from woft_amd import probe
    from woft_amd.tracker import YAOFTrackerSingleControl, make_forward_compatible
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_TRS.py")
    assert conf.tracker_class is YAOFTrackerSingleControl
    assert conf.H_estimator.woft_spec == ("trs", 10000, 3.0, 0.999)
    assert conf.pw_mask and conf.no_prewarp_after_N == 10
    spec, how = probe.solver_spec(conf.H_estimator, make_forward_compatible(conf.subsampler_fn), conf.redet_success_fn)
    assert how.count("tagged") == 3 and spec["trs"] == dict(max_iters=10000, thr=3.0, conf=0.999) and spec["n_draw"] == 500
    with pytest.raises(AssertionError):
        find_homography_TRS(np.zeros((1, 1, 2), np.float32), np.zeros((1, 1, 2), np.float32))
