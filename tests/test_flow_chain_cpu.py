"""Flow sampling, chaining and the forward-backward check on the host: the numpy restatement of the reference
sampler against the reference's own outputs (tests/golden/flow_interp.npz, tools/gen_golden_interp.py), the three new entry points
in the header, EXPORTS and the library, their argument checks, the shim imports, every construction error of the tracker keys
`fb_check` / `fb_alpha` / `fb_beta` (a stub flow provider on DEVICE = "cpu": nothing is computed) and the shipped config."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import flow_chain_host as FH

ROOT = Path(__file__).resolve().parent.parent
NEW = ("woft_sample_bilinear", "woft_flow_chain", "woft_flow_fb")
CASES = ("hand_5x7", "rand_33x65", "row_1x9", "col_9x1")


@pytest.fixture(scope="module")
def gold():
    return np.load(ROOT / "tests" / "golden" / "flow_interp.npz")


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", CASES)
def test_restated_reference_sampler_equals_the_reference_as_bits(gold, case):
    data, x, y = gold[f"{case}_data"], gold[f"{case}_x"], gold[f"{case}_y"]
    assert np.isfinite(x).all() and np.isfinite(y).all() and max(np.abs(x).max(), np.abs(y).max()) <= 1e9
    out = FH.sample_ref32(data, x, y)
    assert out.dtype == np.float32 and np.array_equal(bits(out), bits(gold[f"{case}_interp"]))
    if data.shape[0] == 2:
        warped = (np.stack([x, y]) + out).astype(np.float32)
        assert np.array_equal(bits(warped), bits(gold[f"{case}_warp"]))


def test_fixture_covers_the_edges(gold):
    """The reference's edge rule is in the fixture: on and beyond the last row / column and outside the first, the weights of
    the coinciding corners cancel -- exactly where one coordinate is an integer, else to the rounding of the cancelling terms."""
    x, y, out = gold["hand_5x7_x"], gold["hand_5x7_y"], gold["hand_5x7_interp"]
    edge = (x >= 6) | (y >= 4) | (x < 0) | (y < 0)
    assert edge.sum() >= 8 and np.abs(out[:, edge]).max() < 1e-5
    exact = edge & ((x == np.round(x)) | (y == np.round(y)))
    assert exact.sum() >= 8 and not out[:, exact].any()
    assert np.abs(out[:, ~edge]).min() > 1e-3
    x, y = gold["rand_33x65_x"], gold["rand_33x65_y"]
    inside = (x > 0) & (x < 64) & (y > 0) & (y < 32)
    assert 0.6 < inside.mean() < 0.85 and (x == np.round(x)).sum() >= 1000


def test_edge_exact_restatement_by_hand():
    """The fp64 restatements on a case worked out by hand: f = 2x + 10y sampled exactly (bilinear reproduces it), the last row and
    column return the data there, everything outside is invalid."""
    h, w = 4, 5
    ys, xs = np.mgrid[:h, :w].astype(np.float32)
    fbc = np.stack([2 * xs + 10 * ys, -xs]).astype(np.float32)
    fab = np.zeros((2, h, w), np.float32)
    fab[:, 0, 0] = (0.5, 0.25)          # q = (0.5, 0.25): inside
    fab[:, 3, 4] = (0.0, 0.0)           # q = the last pixel itself: valid, the data there
    fab[:, 1, 4] = (0.001, 0.0)         # just past the last column
    fab[:, 0, 2] = (0.0, -0.001)        # just above the first row
    fab[0, 2, 2] = np.nan
    fac, valid, _ = FH.chain64(fab, fbc)
    assert valid.sum() == h * w - 3 and not valid[1, 4] and not valid[0, 2] and not valid[2, 2]
    assert np.isnan(fac[:, ~valid]).all()
    assert np.allclose(fac[:, 0, 0], (0.5 + 2 * 0.5 + 10 * 0.25, 0.25 - 0.5), rtol=0, atol=1e-12)
    assert np.array_equal(fac[:, 3, 4], (2 * 4 + 10 * 3, -4.0))
    # fb: the reverse flow is the exact negative -> err 0, ok; a planted 1 px disagreement fails beta = 0.5 (1 > 0.5 + 0.01 * ...)
    fwd = np.full((2, h, w), 0.0, np.float32)
    bwd = np.zeros((2, h, w), np.float32)
    bwd[0, 1, 1] = 1.0
    err, ok, _, _, valid = FH.fb64(fwd, bwd, 0.01, 0.5)
    assert valid.all() and ok.sum() == h * w - 1 and not ok[1, 1] and err[1, 1] == 1.0 and err.sum() == 1.0
    fwd[0, 2, 4] = 1.0                  # leaves the frame
    err, ok, _, _, valid = FH.fb64(fwd, bwd, 0.01, 0.5)
    assert not valid[2, 4] and np.isposinf(err[2, 4]) and not ok[2, 4]


def test_test_fields_exercise_every_outcome():
    for h, w in FH.SHAPES:
        fwd, bwd = FH.make_fields(h, w)
        _, ok, _, _, valid = FH.fb64(fwd, bwd, 0.01, 0.5)
        assert valid.any() and ok.any(), (h, w)
        if min(h, w) > 1:
            assert (~valid).any() and (valid & ~ok).any(), (h, w)


def test_header_exports_and_library_agree_on_the_new_names(lib):
    from woft_amd import _lib
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name), name


def test_new_entry_points_reject_bad_arguments_without_a_device(lib):
    """-1 before any launch (host buffers stand in for device ones: nothing is dereferenced)."""
    buf = (ctypes.c_float * 4096)()
    a = ctypes.addressof(buf)
    nan, inf = float("nan"), float("inf")

    def sample(**kw):
        d = dict(dict(data=a, c=2, h=5, w=7, x=a, y=a, n=16, out=a), **kw)
        return lib.woft_sample_bilinear(d["data"], d["c"], d["h"], d["w"], d["x"], d["y"], d["n"], d["out"], None)

    def chain(**kw):
        d = dict(dict(fab=a, fbc=a, h=5, w=7, fac=a), **kw)
        return lib.woft_flow_chain(d["fab"], d["fbc"], d["h"], d["w"], d["fac"], None)

    def fb(**kw):
        d = dict(dict(fab=a, fba=a, h=5, w=7, alpha=0.01, beta=0.5, err=a, ok=a), **kw)
        return lib.woft_flow_fb(d["fab"], d["fba"], d["h"], d["w"], d["alpha"], d["beta"], d["err"], d["ok"], None)

    for bad in (dict(data=None), dict(x=None), dict(y=None), dict(out=None), dict(c=0), dict(c=-1), dict(h=0), dict(w=0),
                dict(h=-3), dict(w=-3), dict(n=-1), dict(h=(1 << 24) + 1), dict(w=(1 << 24) + 1)):
        assert sample(**bad) == -1, bad
    assert sample(n=0) == 0                                   # (no point: nothing is launched)
    for bad in (dict(fab=None), dict(fbc=None), dict(fac=None), dict(h=0), dict(w=0), dict(h=-1), dict(w=-1),
                dict(w=(1 << 24) + 1)):
        assert chain(**bad) == -1, bad
    for bad in (dict(fab=None), dict(fba=None), dict(err=None, ok=None), dict(h=0), dict(w=0), dict(h=-1), dict(w=-1),
                dict(alpha=nan), dict(beta=nan), dict(alpha=-0.01), dict(beta=-1.0), dict(alpha=inf), dict(beta=inf),
                dict(alpha=-inf)):
        assert fb(**bad) == -1, bad


def test_shim_imports_resolve():
    import woft_amd
    from pytracking.utils import interpolation as shim
    from woft_amd import interpolation as own
    for name in ("bilinear_interpolate_torch", "flow_warp_coords", "chain_flow", "fb_consistency"):
        assert getattr(shim, name) is getattr(own, name)
    assert woft_amd.chain_flow is own.chain_flow and woft_amd.fb_consistency is own.fb_consistency
    marker = object()
    assert own.chain_flow(None, marker) is marker             # (interpolation.py:11-12)
    from pytracking.optical_flow.raft import RAFTWrapper
    assert callable(RAFTWrapper.compute_flow_fb)
    with pytest.raises(AttributeError):
        woft_amd.no_such_name


def test_python_layers_reject_bad_constants_before_any_device_work():
    import torch
    from woft_amd.interpolation import fb_consistency
    f = torch.zeros(2, 4, 4)
    for kw in (dict(alpha=-1.0), dict(beta=float("nan")), dict(alpha=float("inf"))):
        with pytest.raises(ValueError, match="alpha and beta"):
            fb_consistency(f, f, **kw)
    with pytest.raises(ValueError, match=r"\(2, H, W\)"):
        fb_consistency(f, torch.zeros(2, 4, 5))


# ---- tracker construction -------------------------------------------------------------------------------------------------------
class _StubProvider:
    def __init__(self, cfg):
        self.C = cfg

    def pin_source(self, img):
        pass

    def flow_map(self):
        raise RuntimeError


class _ForeignProvider:
    def __init__(self, cfg):
        self.C = cfg


@pytest.fixture
def on_cpu(monkeypatch):
    from woft_amd import tracker
    monkeypatch.setattr(tracker.YAOFTrackerSingleControl, "DEVICE", "cpu")
    monkeypatch.delenv("WOFT_FUSED", raising=False)


def _config(name="WOFT_fbcheck.py", provider=_StubProvider, **keys):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / name)
    conf.flow_config.of_class = provider
    for k, v in keys.items():
        setattr(conf, k, v)
    return conf


def test_shipped_config():
    from pytracking.tracker.YAOF_tracker_single_control import YAOFTrackerSingleControl
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_fbcheck.py")
    base = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
    assert conf.tracker_class is YAOFTrackerSingleControl
    assert conf.fb_check == "gate" and conf.fb_alpha == 0.01 and conf.fb_beta == 0.5
    assert not base.fb_check and not conf.visibility_mode
    assert conf.flow_config.raft_type == base.flow_config.raft_type and conf.flow_config.iters == base.flow_config.iters


@pytest.mark.parametrize("raft_type,backend", [("weighted", "device back end"), ("orig", "callable back end")])
def test_valid_config_constructs_and_reports_the_check(on_cpu, raft_type, backend):
    conf = _config(fb_alpha=0.05, fb_beta=1)
    conf.flow_config.raft_type = raft_type
    trk = conf.tracker_class(conf)
    assert (trk.fb_check, trk.fb_alpha, trk.fb_beta) == ("gate", 0.05, 1.0) and trk.visibility_mode is None
    assert trk.solver_decision.startswith(backend) and "forward-backward check gate" in trk.solver_decision
    assert trk._sparse_weights is False and trk._flow_region_on() is False       # (the un-pruned path)
    trk = (lambda c: c.tracker_class(c))(_config())
    assert (trk.fb_alpha, trk.fb_beta) == (0.01, 0.5)
    conf = _config()
    del conf.fb_alpha, conf.fb_beta
    trk = conf.tracker_class(conf)
    assert (trk.fb_alpha, trk.fb_beta) == (0.01, 0.5)                             # (the defaults)


@pytest.mark.parametrize("off", ["absent", None, False, ""])
def test_no_key_leaves_the_tracker_as_it_was(on_cpu, off):
    conf = _config("WOFT.py", provider=_ForeignProvider)
    if off != "absent":
        conf.fb_check = off
    trk = conf.tracker_class(conf)
    assert trk.fb_check is None and "forward-backward" not in trk.solver_decision


@pytest.mark.parametrize("keys,match", [
    (dict(fb_check="weight"), "fb_check"),                                        # 'gate' is the only mode
    (dict(fb_check=True), "fb_check"),
    (dict(fb_check=1), "fb_check"),
    (dict(fb_alpha=-0.01), "fb_alpha"),
    (dict(fb_alpha=float("nan")), "fb_alpha"),
    (dict(fb_alpha=float("inf")), "fb_alpha"),
    (dict(fb_alpha="small"), "fb_alpha"),
    (dict(fb_beta=-1), "fb_beta"),
    (dict(fb_beta=float("nan")), "fb_beta"),
    (dict(fb_beta=[0.5]), "fb_beta"),
])
def test_bad_keys_raise_at_construction(on_cpu, keys, match):
    conf = _config(**keys)
    with pytest.raises(ValueError, match=match):
        conf.tracker_class(conf)


@pytest.mark.parametrize("mode", ["gate", "weight"])
def test_fb_check_with_a_visibility_mode_raises(on_cpu, mode):
    conf = _config("WOFT_visibility.py", fb_check="gate", visibility_mode=mode)
    with pytest.raises(ValueError, match="one visibility slot"):
        conf.tracker_class(conf)


def test_window_tracker_refuses_fb_check(on_cpu):
    from woft_amd.tracker import WOFTWindow
    conf = _config("WOFT_window.py", fb_check="gate")
    with pytest.raises(NotImplementedError, match="fb_check"):
        WOFTWindow(conf)
    conf = _config("WOFT_window.py")                                              # (without the key: as before)
    assert WOFTWindow(conf).fb_check is None


def test_a_provider_without_the_flow_map_is_refused(on_cpu):
    conf = _config(provider=_ForeignProvider)
    with pytest.raises(NotImplementedError, match="fb_check"):
        conf.tracker_class(conf)
