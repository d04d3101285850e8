"""The tracker's visibility modes on the host (DESIGN.md "Visibility mask in the tracker"): the two new entry points in the header
and the library, every construction error of the tracker config keys `visibility_mode` / `visibility_thr` (a stub flow provider on
DEVICE = "cpu": nothing is computed), the shipped config, and the numpy restatement of the two rules (tests/visibility_host.py) on a
6 x 8 case whose expected flags and weights are written out by hand."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import visibility_host as V

ROOT = Path(__file__).resolve().parent.parent
NEW = ("woft_tc_select_vis", "woft_tc_flags_vis")


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_declares_and_library_exports_the_new_entry_points(lib):
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
    sel = dict(dst=a, w=a, tmask=a, pwmask=None, gh=6, gw=8, mh=6, mw=8, check_dst=1, u=a, n_draw=4, vis=a, mode=1, thr=0.5, ws=a,
               pa=a, pb=a, wout=a, cap=48, count=a)

    def select(**kw):
        d = dict(sel, **kw)
        return lib.woft_tc_select_vis(d["dst"], d["w"], d["tmask"], d["pwmask"], d["gh"], d["gw"], d["mh"], d["mw"], d["check_dst"],
                                      d["u"], d["n_draw"], d["vis"], d["mode"], d["thr"], d["ws"], d["pa"], d["pb"], d["wout"],
                                      d["cap"], d["count"], None)

    def flags(**kw):
        d = dict(sel, **kw)
        return lib.woft_tc_flags_vis(d["dst"], d["tmask"], d["pwmask"], d["gh"], d["gw"], d["mh"], d["mw"], d["check_dst"], d["vis"],
                                     d["mode"], d["thr"], d["pa"], None)

    for bad in (dict(mode=3), dict(mode=-1), dict(thr=float("nan")), dict(tmask=None), dict(gh=7), dict(gw=9), dict(gh=0),
                dict(dst=None)):
        assert select(**bad) == -1, bad
        assert flags(**bad) == -1, bad
    for bad in (dict(ws=None), dict(pa=None), dict(pb=None), dict(count=None), dict(cap=0), dict(n_draw=1025), dict(u=None)):
        assert select(**bad) == -1, bad


# ---- tracker construction -------------------------------------------------------------------------------------------------------
class _StubProvider:
    def __init__(self, cfg):
        self.C = cfg

    def pin_source(self, img):
        pass


@pytest.fixture
def on_cpu(monkeypatch):
    from woft_amd import tracker
    monkeypatch.setattr(tracker.YAOFTrackerSingleControl, "DEVICE", "cpu")
    monkeypatch.delenv("WOFT_FUSED", raising=False)


def _config(name="WOFT_visibility.py", **keys):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / name)
    conf.flow_config.of_class = _StubProvider
    for k, v in keys.items():
        setattr(conf, k, v)
    return conf


def test_shipped_config():
    from pytracking.tracker.YAOF_tracker_single_control import YAOFTrackerSingleControl
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_visibility.py")
    base = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
    assert conf.tracker_class is YAOFTrackerSingleControl and conf.visibility_mode == "gate"
    fc = conf.flow_config
    assert fc.raft_type == "weighted_masked" and fc.class_params.mask_estimation is True
    assert [tuple(d) for d in fc.class_params.mask_head_structure] == [(128, 3), (128, 3)]
    assert base.flow_config.raft_type == "weighted" and not base.visibility_mode
    assert conf.no_prewarp_after_N == base.no_prewarp_after_N and fc.iters == base.flow_config.iters


@pytest.mark.parametrize("mode", ["gate", "weight"])
def test_valid_config_constructs_and_reports_its_mode(on_cpu, mode):
    conf = _config(visibility_mode=mode, visibility_thr=0.25)
    trk = conf.tracker_class(conf)
    assert trk.visibility_mode == mode and trk.visibility_thr == float(np.float32(0.25))
    assert trk.solver_decision.startswith("device back end") and f"visibility {mode}" in trk.solver_decision
    assert trk._fused is not None and trk._sparse_weights is False
    conf = _config(visibility_mode=mode, device_solver=False)
    trk = conf.tracker_class(conf)
    assert trk.solver_decision.startswith("callable back end") and f"visibility {mode}" in trk.solver_decision
    assert trk._fused is None and trk.visibility_thr == 0.5                       # (the default threshold)


def test_threshold_is_rounded_to_fp32_once(on_cpu):
    conf = _config(visibility_thr=0.1)
    trk = conf.tracker_class(conf)
    assert trk.visibility_thr == float(np.float32(0.1)) != 0.1


@pytest.mark.parametrize("keys,match", [
    (dict(visibility_mode="mask"), "visibility_mode"),                           # not a mode
    (dict(visibility_mode=1), "visibility_mode"),
    (dict(visibility_mode="gate", visibility_thr=0.0), "visibility_thr"),        # outside (0, 1)
    (dict(visibility_mode="gate", visibility_thr=1.0), "visibility_thr"),
    (dict(visibility_mode="weight", visibility_thr=-0.5), "visibility_thr"),
    (dict(visibility_mode="gate", visibility_thr=float("nan")), "visibility_thr"),
    (dict(visibility_mode="gate", visibility_thr="high"), "visibility_thr"),
])
def test_bad_keys_raise_at_construction(on_cpu, keys, match):
    conf = _config(**keys)
    with pytest.raises(ValueError, match=match):
        conf.tracker_class(conf)


@pytest.mark.parametrize("raft_type", ["orig", "weighted"])
@pytest.mark.parametrize("mode", ["gate", "weight"])
def test_a_mode_without_a_masked_flow_config_raises(on_cpu, raft_type, mode):
    conf = _config("WOFT.py", visibility_mode=mode)
    conf.flow_config.raft_type = raft_type
    with pytest.raises(ValueError, match="weighted_masked"):
        conf.tracker_class(conf)


@pytest.mark.parametrize("off", ["absent", None, False, ""])
def test_masked_flow_config_without_a_mode_still_raises_the_old_error(on_cpu, off):
    conf = _config()
    if off == "absent":
        del conf.visibility_mode
        assert not conf.visibility_mode
    else:
        conf.visibility_mode = off
    with pytest.raises(ValueError, match="does not consume"):
        conf.tracker_class(conf)


def test_no_mode_leaves_the_weighted_tracker_as_it_was(on_cpu):
    conf = _config("WOFT.py")
    trk = conf.tracker_class(conf)
    assert trk.visibility_mode is None and "visibility" not in trk.solver_decision
    assert trk.solver_decision.startswith("device back end")


# ---- the rules, by hand ---------------------------------------------------------------------------------------------------------
GH, GW, THR = 6, 8, 0.5
NAN = float("nan")


def _hand_case():
    """Identity flow on a 6 x 8 grid, template mask = rows 1-4 x columns 1-6; one target out of bounds; p = 0.9 except the planted
    values: exactly thr, NaN, 0.25 and 0 inside the mask, 1.0 on a pixel outside it and on the mask's last pixel."""
    ys, xs = np.mgrid[0:GH, 0:GW]
    dst = np.stack([xs.ravel(), ys.ravel()]).astype(np.float32)
    dst[0, 2 * GW + 3] = -1.0                                   # (2, 3) leaves the frame
    tmask = np.zeros((GH, GW), np.uint8)
    tmask[1:5, 1:7] = 255
    p = np.full((GH, GW), 0.9, np.float32)
    p[1, 1] = THR
    p[1, 2] = NAN
    p[3, 3] = 0.25
    p[2, 5] = 0.0
    p[0, 0] = 1.0                                               # outside the mask: stays out
    p[4, 6] = 1.0
    w = ((np.arange(GH * GW) + 1) / 64.0).astype(np.float32)   # exact in fp32
    return dst, tmask, p.ravel(), w


PLAIN = np.array([[0, 0, 0, 0, 0, 0, 0, 0],
                  [0, 1, 1, 1, 1, 1, 1, 0],
                  [0, 1, 1, 0, 1, 1, 1, 0],
                  [0, 1, 1, 1, 1, 1, 1, 0],
                  [0, 1, 1, 1, 1, 1, 1, 0],
                  [0, 0, 0, 0, 0, 0, 0, 0]], bool)
GATED = np.array([[0, 0, 0, 0, 0, 0, 0, 0],
                  [0, 0, 0, 1, 1, 1, 1, 0],                     # p == thr and NaN p: dropped
                  [0, 1, 1, 0, 1, 0, 1, 0],                     # out-of-bounds target; p = 0
                  [0, 1, 1, 0, 1, 1, 1, 0],                     # p = 0.25
                  [0, 1, 1, 1, 1, 1, 1, 0],
                  [0, 0, 0, 0, 0, 0, 0, 0]], bool)


def test_gate_by_hand():
    dst, tmask, p, w = _hand_case()
    assert np.array_equal(V.keep_rule_vis(dst, tmask, None, GH, GW, None, V.GATE, THR).reshape(GH, GW), PLAIN)
    assert np.array_equal(V.keep_rule_vis(dst, tmask, None, GH, GW, p, V.WEIGHT, THR).reshape(GH, GW), PLAIN)
    keep = V.keep_rule_vis(dst, tmask, None, GH, GW, p, V.GATE, THR).reshape(GH, GW)
    assert np.array_equal(keep, GATED)
    assert not keep[1, 1] and not keep[1, 2]                    # p exactly thr; NaN p
    pa, pb, wo, m, n_kept = V.select_vis(dst, w, tmask, None, GH, GW, np.zeros(0, np.float32), 48, p, V.GATE, THR)
    assert (m, n_kept) == (19, 19) == (int(GATED.sum()),) * 2
    idx = np.flatnonzero(GATED.ravel())
    assert np.array_equal(pb, np.stack([idx % GW, idx // GW], 1).astype(np.float32)) and np.array_equal(pa, pb)
    assert np.array_equal(wo, w[idx])                           # weights untouched
    # a threshold just under the planted value keeps it: the compare is strict, on the fp32 values
    below = np.nextafter(np.float32(THR), np.float32(0))
    assert V.keep_rule_vis(dst, tmask, None, GH, GW, p, V.GATE, below).reshape(GH, GW)[1, 1]
    # a draw runs on the gated set: 4 Sobol points -> ranks rint(19 * u)
    u = np.array([0.0, 0.5, 0.75, 0.25], np.float32)
    _, pb4, _, m4, n4 = V.select_vis(dst, w, tmask, None, GH, GW, u, 48, p, V.GATE, THR)
    assert (m4, n4) == (4, 19)
    pick = idx[[0, 5, 10, 14]]                                  # rint(0), rint(4.75), rint(9.5) = 10 (half to even), rint(14.25)
    assert np.array_equal(pb4, np.stack([pick % GW, pick // GW], 1).astype(np.float32))


def test_weight_by_hand():
    dst, tmask, p, w = _hand_case()
    pa, pb, wo, m, n_kept = V.select_vis(dst, w, tmask, None, GH, GW, np.zeros(0, np.float32), 48, p, V.WEIGHT, THR)
    assert (m, n_kept) == (23, 23) == (int(PLAIN.sum()),) * 2
    idx = np.flatnonzero(PLAIN.ravel())
    assert wo.dtype == np.float32
    want = {(1, 1): 10 / 64 * 0.5, (2, 5): 0.0, (3, 3): 28 / 64 * 0.25, (4, 6): 39 / 64 * 1.0,
            (1, 3): float(np.float32(12 / 64) * np.float32(0.9))}
    for (y, x), v in want.items():
        k = int(np.flatnonzero(idx == y * GW + x)[0])
        assert wo[k] == np.float32(v), (y, x, wo[k], v)
    k_nan = int(np.flatnonzero(idx == 1 * GW + 2)[0])
    assert np.isnan(wo[k_nan]) and np.isfinite(np.delete(wo, k_nan)).all()      # a NaN p is the caller's to gate: it propagates
    # without weights the output weight is p itself
    _, _, wo_p, _, _ = V.select_vis(dst, None, tmask, None, GH, GW, np.zeros(0, np.float32), 48, p, V.WEIGHT, THR)
    assert np.array_equal(wo_p, p[idx], equal_nan=True)
    # ... and in gate mode / without a mask it is the plain selection's: ones
    _, _, wo_1, _, _ = V.select_vis(dst, None, tmask, None, GH, GW, np.zeros(0, np.float32), 48, p, V.GATE, THR)
    assert np.array_equal(wo_1, np.ones(19, np.float32))
