"""Warm start without a GPU: the numpy restatement (tests/warm_host.py) against the reference's own
forward_interpolate outputs (tests/golden/warm_start_128x160_it4.npz, tools/gen_golden_warm.py), argument checks of the two
entry points, the config and the window tracker's refusal."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import warm_host  # noqa: E402

FI_CASES = ["small_16x20", "large_16x20", "odd_17x23", "one_valid_16x20"]


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir / "warm_start_128x160_it4.npz")


def test_fixture_holds_the_four_cases(gold):
    assert sorted(FI_CASES) == sorted(str(n) for n in gold["fi_names"])
    assert int(gold["fi_one_valid_16x20_valid"]) == 1
    n, total = int(gold["fi_large_16x20_valid"]), gold["fi_large_16x20_flow"][0].size
    assert 0.3 * total < n < 0.7 * total                  # "about half the points leave the grid"
    assert gold["fi_odd_17x23_flow"].shape == (2, 17, 23)


@pytest.mark.parametrize("name", FI_CASES)
def test_warm_host_equals_the_reference(gold, name):
    out = warm_host.forward_interpolate(gold[f"fi_{name}_flow"])
    assert out.dtype == np.float32 and np.array_equal(out, gold[f"fi_{name}_out"])


def test_warm_host_tie_and_empty_rules():
    # two points land at the same distance from cell (1, 1): the lower index wins
    f = np.full((2, 3, 3), 100.0, np.float32)             # everything else leaves the grid
    f[:, 0, 1] = (-0.5, 1.0)                              # point 1 (x0 = 1, y0 = 0) -> (0.5, 1.0)
    f[:, 2, 1] = (0.5, -1.0)                              # point 7 (x0 = 1, y0 = 2) -> (1.5, 1.0)
    out = warm_host.forward_interpolate(f)
    assert tuple(out[:, 1, 1]) == (-0.5, 1.0)
    # on the border is outside: x1 = 0 exactly is not valid
    g = np.full((2, 3, 3), 100.0, np.float32)
    g[:, 1, 1] = (-1.0, 0.0)
    assert not warm_host.forward_interpolate(g).any()
    assert not warm_host.forward_interpolate(np.full((2, 4, 5), np.nan, np.float32)).any()


def test_coords_init_flow_host():
    f = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4) / 7
    coords, flow = warm_host.coords_init_flow(f)
    assert coords.shape == (12, 2) and np.array_equal(flow[:, 0], f[0].ravel()) and np.array_equal(flow[:, 1], f[1].ravel())
    assert coords[5, 0] == np.float32(1) + f[0, 1, 1] and coords[5, 1] == np.float32(1) + f[1, 1, 1]


def test_entry_points_reject_bad_arguments(lib):
    buf = (ctypes.c_float * 64)()
    buf2 = (ctypes.c_float * 64)()
    p, q = ctypes.addressof(buf), ctypes.addressof(buf2)
    ci = lib.woft_coords_init_flow
    assert ci(None, p, 2, 2, None, None, 0, None) == -1
    assert ci(p, None, 2, 2, None, None, 0, None) == -1
    for hf, wf in ((0, 2), (2, 0), (-1, 2), (2, -3)):
        assert ci(p, q, hf, wf, None, None, 0, None) == -1
    fi = lib.woft_forward_interpolate
    assert fi(None, 2, 2, q, None) == -1 and fi(p, 2, 2, None, None) == -1
    assert fi(p, 2, 2, p, None) == -1                      # in place
    for hf, wf in ((0, 2), (2, 0), (-1, 2), (2, -3), (1 << 16, 1 << 16)):
        assert fi(p, hf, wf, q, None) == -1


def test_header_and_exports():
    from woft_amd import _lib
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    assert {"woft_coords_init_flow", "woft_forward_interpolate"} <= declared
    assert {"woft_coords_init_flow", "woft_forward_interpolate"} <= set(_lib.EXPORTS)


def test_config_loads_and_the_probe_keeps_the_device_back_end():
    from pytracking.tracker.YAOF_tracker_single_control import YAOFTrackerSingleControl
    from pytracking.utils.config import load_config
    from woft_amd.probe import solver_spec
    from woft_amd.tracker import make_forward_compatible
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_warmstart.py")
    base = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
    assert conf.tracker_class is YAOFTrackerSingleControl and conf.warm_start_local is True
    assert not base.warm_start_local and not base.warm_start_iters and not conf.warm_start_iters
    a = solver_spec(conf.H_estimator, make_forward_compatible(conf.subsampler_fn), conf.redet_success_fn, device="cpu")
    b = solver_spec(base.H_estimator, make_forward_compatible(base.subsampler_fn), base.redet_success_fn, device="cpu")
    assert a[0] is not None and a == b


def test_window_tracker_refuses_the_key():
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_window.py")
    conf.warm_start_local = True
    with pytest.raises(NotImplementedError, match="warm_start_local"):
        conf.tracker_class(conf)


def test_warm_start_iters_is_validated():
    from types import SimpleNamespace
    from pytracking.utils.config import load_config
    from woft_amd.tracker import YAOFTrackerSingleControl
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_warmstart.py")
    for bad in (0, -2, 1.5, "3", True):
        conf.warm_start_iters = bad
        with pytest.raises(ValueError, match="warm_start_iters"):
            YAOFTrackerSingleControl._warm_start_config(SimpleNamespace(C=conf))
    conf.warm_start_iters = 6
    assert YAOFTrackerSingleControl._warm_start_config(SimpleNamespace(C=conf)) == (True, 6)


def test_package_exports_forward_interpolate():
    from woft_amd import forward_interpolate
    from woft_amd.warm import forward_interpolate as f
    assert forward_interpolate is f
    with pytest.raises(TypeError):
        forward_interpolate(np.zeros((2, 4, 4), np.float32))
