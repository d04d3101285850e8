"""The RANSAC estimator without a GPU: its C ABI entries reject bad arguments before touching the device, header and exports
agree, the probe recognises a reference-form RANSAC config (tests/configs/reference_forms_ransac.py), the preset is tagged and
the shim config loads."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_ransac_abi_rejects_bad_arguments(lib):
    buf = (ctypes.c_float * 64)()
    st = (ctypes.c_int32 * 4)()
    p = ctypes.addressof(buf)
    s = ctypes.addressof(st)
    ok = dict(pa=p, pb=p, n_max=8, count=None, max_iters=100, thr=3.0, conf=0.995, seed=0, refine=1, ws=p, Hout=p, status=s,
              info=None, mask=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.woft_ransac(a["pa"], a["pb"], a["n_max"], a["count"], a["max_iters"], a["thr"], a["conf"], a["seed"],
                               a["refine"], a["ws"], a["Hout"], a["status"], a["info"], a["mask"], a["stream"])
    for bad in (dict(pa=None), dict(pb=None), dict(ws=None), dict(Hout=None), dict(status=None), dict(n_max=-1),
                dict(max_iters=0), dict(max_iters=-5), dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")),
                dict(conf=-0.01), dict(conf=1.01), dict(conf=float("nan"))):
        assert call(**bad) == -1, bad
    assert lib.woft_ransac_ws_bytes(-1, 10) == -1 and lib.woft_ransac_ws_bytes(10, 0) == -1
    small, big = lib.woft_ransac_ws_bytes(500, 10000), lib.woft_ransac_ws_bytes(2073600, 200)
    assert small >= 4 * (500 + 10000) and big >= 4 * 2073600 + lib.woft_hfit_ws_bytes()


def test_ransac_header_and_exports(lib):
    from woft_amd import _lib
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    assert {"woft_ransac", "woft_ransac_ws_bytes"} <= declared
    assert declared == set(_lib.EXPORTS)
    assert lib.woft_abi_version() == 400


def test_probe_recognises_the_reference_form_ransac_config():
    from woft_amd import probe
    from woft_amd.tracker import make_forward_compatible
    sys.dont_write_bytecode = True
    path = ROOT / "tests" / "configs" / "reference_forms_ransac.py"
    import types
    m = types.ModuleType("tracker_config")
    m.__file__ = str(path)
    exec(compile(path.read_text(), str(path), "exec"), m.__dict__)
    conf = m.get_config()
    assert probe.probe_estimator(conf.H_estimator) == ("ransac", 10000, 3.0, 0.995, False)
    spec, how = probe.solver_spec(conf.H_estimator, make_forward_compatible(conf.subsampler_fn), conf.redet_success_fn)
    assert spec is not None and how.count("probed") == 3, how
    assert spec["ransac"] == dict(max_iters=10000, thr=3.0, conf=0.995) and spec["weighted"] is False
    assert (spec["thr"], spec["min_frac"], spec["n_draw"], spec["const_verdict"]) == (5.0, 0.2, 500, None)


def test_probe_rejects_ransac_forms_it_cannot_run():
    from woft_amd import probe
    from woft_amd.homography import find_homography_cvransac as ransac
    assert probe.probe_estimator(lambda a, b, weights=None: ransac(a, b)) == ("ransac", 10000, 1.4142, 0.995, False)
    assert probe.probe_estimator(lambda a, b, weights=None: ransac(a, b, max_iters=a.shape[1] * 10)) is None   # not constant
    assert probe.probe_estimator(lambda a, b, weights=None: ransac(a, b, max_iters=100.5)) is None
    assert probe.probe_estimator(lambda a, b, weights=None: ransac(a, b, thr=-1)) is None
    assert probe.probe_estimator(lambda a, b, weights=None: ransac(a * 2, b)) is None
    assert probe.probe_estimator(lambda a, b, weights=None: ransac(a, b) * 1.0) is None


def test_ransac_preset_is_tagged_and_probe_agrees():
    from woft_amd import presets, probe
    est = presets.estimator_ransac()
    assert est.woft_spec == ("ransac", 10000, 3.0, 0.995)
    assert probe.probe_estimator(est) == ("ransac", 10000, 3.0, 0.995, False)
    est = presets.estimator_ransac(max_iters=2000, thr=2.5, conf=0.99)
    assert probe.probe_estimator(est) == ("ransac", 2000, 2.5, 0.99, False)


def test_ransac_shim_config_loads():
    from pytracking.utils.config import load_config
    from pytracking.utils.least_squares_H import find_homography_cvransac
    from woft_amd import probe
    from woft_amd.tracker import YAOFTrackerSingleControl, make_forward_compatible
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_RANSAC.py")
    assert conf.tracker_class is YAOFTrackerSingleControl
    assert conf.H_estimator.woft_spec == ("ransac", 10000, 3.0, 0.995)
    assert conf.pw_mask and conf.no_prewarp_after_N == 10
    spec, how = probe.solver_spec(conf.H_estimator, make_forward_compatible(conf.subsampler_fn), conf.redet_success_fn)
    assert how.count("tagged") == 3 and spec["ransac"] == dict(max_iters=10000, thr=3.0, conf=0.995) and spec["n_draw"] == 500
    with pytest.raises(AssertionError):
        find_homography_cvransac(np.zeros((1, 3, 2), np.float32), np.zeros((1, 3, 2), np.float32))
