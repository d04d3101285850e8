"""The planar tracker on chained flow, on the host: the new entry point in the header, EXPORTS and the library,
its argument checks (-1 before any device work), the numpy restatement in both dtypes, every construction error of WOFTChained, its
shipped config, and its state machine around a stubbed fold, a stubbed chain_tc and a stubbed solver (nothing is computed)."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import chain_tc_host as CH

ROOT = Path(__file__).resolve().parent.parent
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_exports_and_library_agree_on_the_new_name(lib):
    from woft_amd import _lib, ops
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    name = "woft_chain_tc"
    assert name in declared and name in _lib.EXPORTS and hasattr(raw, name)
    assert len(_lib._SIGS[name][1]) == 15
    assert re.search(r"^#define\s+WOFT_CHAIN_HIST\s+130\s*$", header, flags=re.M) and ops.CHAIN_HIST == CH.HIST == 130


def test_chain_tc_rejects_bad_arguments_without_a_device(lib):
    """-1 before any launch (host buffers stand in for device ones: nothing is dereferenced).  Every plane of the base call is a
    buffer of its own, so each case has exactly one thing wrong."""
    gh, gw, mh, mw = 5, 7, 6, 9
    buf = (ctypes.c_float * 8192)()
    base = ctypes.addressof(buf)
    at = lambda j: base + 4 * 512 * j                         # (2 KiB apart: a 5 x 7 flow is 280 B, the histogram 520 B)
    good = dict(flow=at(0), cost=at(1), vis=at(2), sel=at(3), tmask=at(4), gh=gh, gw=gw, mh=mh, mw=mw, vis_thr=0.5, dst=at(5),
                w=at(6), ok=at(7), hist=at(8))
    order = list(good)

    def call(**kw):
        d = dict(good, **kw)
        return lib.woft_chain_tc(*[d[n] for n in order], None)

    plane = 4 * gh * gw
    ins = dict(flow=2 * plane, cost=plane, vis=plane, sel=plane, tmask=mh * mw)
    outs = dict(dst=2 * plane, w=plane, ok=plane, hist=4 * 130)
    bad = [dict(flow=None), dict(cost=None), dict(vis=None), dict(sel=None), dict(dst=None), dict(ok=None),
           dict(gh=0), dict(gw=0), dict(gh=-1), dict(gw=-5), dict(gh=(1 << 24) + 1), dict(gw=(1 << 24) + 1),
           dict(mh=gh - 1), dict(mw=gw - 1), dict(mh=0), dict(mw=-1),
           dict(vis_thr=-0.01), dict(vis_thr=1.01), dict(vis_thr=NAN), dict(vis_thr=INF), dict(vis_thr=-INF)]
    # every output against every input, at the input's first and last byte, and against every other output
    for o, no in outs.items():
        for i, ni in ins.items():
            bad += [{o: good[i]}, {o: good[i] + ni - 1}, {o: good[i] - no + 1}]
        for p, np_ in outs.items():
            if p != o:
                bad += [{o: good[p]}, {o: good[p] + np_ - 1}]
    bad += [dict(dst=good["flow"] + plane), dict(ok=good["flow"] + 2 * plane - 4), dict(w=good["dst"] + plane),
            dict(hist=good["dst"] + 2 * plane - 4)]
    # (only refused calls are made here: an accepted one would launch on these host buffers.  That the optional pointers, the
    #  closed ends of the threshold's range and a mask of the grid's own size are accepted is test_chained_gpu.py's part)
    for kw in bad:
        assert call(**kw) == -1, kw


@pytest.mark.parametrize("case", CH.CASES)
def test_restatement_agrees_between_float32_and_float64(case):
    """ok and hist are decided by exact compares: the dtype of the restatement cannot move them; dst is the fp32 sum in both."""
    h, w, K, mask_hw = case
    for thr in (0.5, 0.3):
        c = CH.make_case(h, w, K, mask_hw=mask_hw, vis_thr=thr)
        r64 = CH.chain_tc(c["flow"], c["cost"], c["vis"], c["sel"], c["mask"], thr)
        r32 = CH.chain_tc(c["flow"], c["cost"], c["vis"], c["sel"], c["mask"], thr, dtype=np.float32)
        assert np.array_equal(r64["ok"], r32["ok"]) and np.array_equal(r64["hist"], r32["hist"])
        assert np.array_equal(r64["dst"].astype(np.float32), r32["dst"], equal_nan=True)
        assert r64["hist"].sum() == (c["mask"][:h, :w] != 0).sum()
        # the planted pixels: which are valid, which are visible
        for i, name, v in c["planted"]:
            valid = name == "vis" and v == np.float32(thr) or name == "sel" and v == 127
            assert bool(r64["valid"].reshape(-1)[i]) == valid and r64["ok"][0, i] == float(valid), (i, name, v)
            assert np.isnan(r64["dst"][:, i]).all() == (not valid) and (r64["w"][0, i] == 0) == (not valid)
        assert r64["hist"][127] == 1 and r64["hist"][CH.INVALID] == len(CH.PLANTS) - 2
    n = CH.chain_tc(c["flow"], c["cost"], c["vis"], c["sel"], None, thr)
    assert n["hist"].sum() == h * w


def test_restatement_by_hand():
    """2 x 3, threshold 0.5: pixel 0 visible with sel 1, pixel 1 at the threshold (visible), pixel 2 below it, pixel 3 without a
    chain, pixel 4 with an infinite cost, pixel 5 visible but outside the mask."""
    flow = np.array([[[1, 2, 3], [4, 5, 6]], [[-1, 0, 1], [0.5, 0.25, -2]]], np.float32)
    cost = np.array([[0, 1, 2], [3, INF, 0.5]], np.float32)
    vis = np.array([[1, 0.5, 0.4999], [0.9, 0.9, 0.9]], np.float32)
    sel = np.array([[1, 0, 0], [-1, 2, 3]], np.int32)
    mask = np.array([[1, 1, 255], [1, 1, 0]], np.uint8)
    for dtype in (np.float64, np.float32):
        r = CH.chain_tc(flow, cost, vis, sel, mask, 0.5, dtype=dtype)
        assert r["ok"].tolist() == [[1, 1, 0, 0, 0, 1]]
        assert r["dst"][:, :3].tolist() == [[1, 3, 5], [-1, 0, 1]] and np.isnan(r["dst"][:, 3:5]).all()
        assert r["dst"][:, 5].tolist() == [8, -1]
        assert np.allclose(r["w"][0], [1, np.exp(-1), np.exp(-2), 0, 0, np.exp(-0.5)], rtol=1e-6, atol=0)
        want = np.zeros(130, np.int32)
        want[[0, 1, 128, 129]] = [1, 1, 2, 1]
        assert np.array_equal(r["hist"], want)


# ---- construction ---------------------------------------------------------------------------------------------------------------
class _StubProvider:
    """Has what the chained tracker asks of a provider; a 'flow' is a zero map."""

    def __init__(self, cfg):
        self.C = cfg
        self.pinned, self.calls = None, 0

    def pin_source(self, img):
        self.pinned = img

    def compute_flow(self, src, dst, mode=None, do_sigmoid=None, borrow=None, **kw):
        import torch
        assert mode == "flow" and do_sigmoid is False and borrow is True
        self.calls += 1
        return torch.zeros(2, *src.shape[:2]), None


class _NoPinProvider:
    def __init__(self, cfg):
        self.C = cfg


@pytest.fixture
def on_cpu(monkeypatch):
    from woft_amd import multiflow, tracker
    monkeypatch.setattr(tracker.YAOFTrackerSingleControl, "DEVICE", "cpu")
    monkeypatch.setattr(multiflow.MultiFlowTracker, "DEVICE", "cpu")
    monkeypatch.delenv("WOFT_FUSED", raising=False)


def _config(provider=_StubProvider, flow_keys=None, **keys):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained.py")
    conf.flow_config.of_class = provider
    for k, v in (flow_keys or {}).items():
        setattr(conf.flow_config, k, v)
    for k, v in keys.items():
        setattr(conf, k, v)
    return conf


def test_shipped_config_and_exports():
    import woft_amd
    from pytracking.tracker.WOFT_chained import WOFTChained
    from pytracking.utils.config import load_config
    from woft_amd import chained
    from woft_amd.tracker import YAOFTrackerSingleControl
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained.py")
    base = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
    assert conf.tracker_class is WOFTChained is chained.WOFTChained is woft_amd.WOFTChained
    assert issubclass(WOFTChained, YAOFTrackerSingleControl)
    assert woft_amd.chain_correspondences is chained.chain_correspondences
    assert tuple(conf.chain_deltas) == (None, 1, 2, 4, 8, 16, 32) == chained.DEFAULT_DELTAS
    assert (conf.chain_vis_thr, conf.chain_unit_cost, conf.chain_iters, conf.chain_weights) == (0.5, 1.0, None, True)
    assert conf.flow_config.raft_type == base.flow_config.raft_type == "weighted" and conf.flow_config.iters == base.flow_config.iters
    # the demo loads a config by its path and builds config.tracker_class: nothing there names a tracker
    demo = (ROOT / "tools" / "woft_demo_headless.py").read_text()
    assert "load_config(config_path)" in demo and "config.tracker_class(config)" in demo


def test_defaults_and_solver_decision(on_cpu):
    conf = _config()
    for k in ("chain_deltas", "chain_vis_thr", "chain_unit_cost", "chain_iters", "chain_weights"):
        delattr(conf, k)                                                       # (every chain key is optional)
    trk = conf.tracker_class(conf)
    assert trk.chain_deltas == (None, 1, 2, 4, 8, 16, 32) and trk.multi.deltas == trk.chain_deltas
    assert (trk.multi.vis_thr, trk.multi.unit_cost, trk.multi.iters, trk.chain_weights) == (0.5, 1.0, None, True)
    assert (trk._vis_mode, trk._vis_thr) == ("gate", 0.5) and trk.visibility_mode is None and not trk.fb_check
    d = trk.solver_decision
    assert d.startswith("device back end") and "(None, 1, 2, 4, 8, 16, 32)" in d
    assert all(k in d for k in ("pw_mask", "no_prewarp_after_N", "no_local_H", "do_not_mask_TCs_by_prewarped")) and "not used" in d
    assert trk._fused is not None and trk._fused.get("weighted", True) and trk._wants_weights()
    trk = _config(chain_deltas=[None, 3], chain_vis_thr=0.25, chain_unit_cost=2.0, chain_iters=5, chain_weights=False)
    trk = trk.tracker_class(trk)
    assert trk.chain_deltas == (None, 3) and (trk.multi.vis_thr, trk.multi.unit_cost, trk.multi.iters) == (0.25, 2.0, 5)
    assert trk._fused["weighted"] is False and not trk._wants_weights() and "(None, 3)" in trk.solver_decision
    trk = _config(device_solver=False)
    trk = trk.tracker_class(trk)
    assert trk._fused is None and trk.solver_decision.startswith("callable back end") and trk._wants_weights()


@pytest.mark.parametrize("raft_type", ["orig", "weighted", "weighted_masked"])
def test_every_raft_type_constructs_with_the_device_solver(on_cpu, raft_type):
    """'weighted_masked' WITHOUT a visibility_mode: the fold consumes the mask (the parent class still refuses it)."""
    from woft_amd.tracker import YAOFTrackerSingleControl
    conf = _config(flow_keys=dict(raft_type=raft_type))
    trk = conf.tracker_class(conf)
    assert trk._fused is not None and trk.solver_decision.startswith("device back end")
    if raft_type == "weighted_masked":
        with pytest.raises(ValueError, match="does not consume"):
            YAOFTrackerSingleControl(conf)


@pytest.mark.parametrize("keys,match", [
    (dict(visibility_mode="gate"), "visibility_mode"), (dict(visibility_mode="weight"), "visibility_mode"),
    (dict(fb_check="gate"), "fb_check"), (dict(warm_start_local=True), "warm_start_local"),
    (dict(downscale_inputs=2), "downscale_inputs"), (dict(search_window_margin=0.25), "search_window_margin"),
    (dict(post_hoc_weights_postprocessing_fn=lambda w: w), "post_hoc_weights_postprocessing_fn"),
    (dict(flow_keys=dict(weights_postprocessing_fn=lambda w: w)), "weights_postprocessing_fn"),
    (dict(provider=_NoPinProvider), "pin_source"),
])
def test_refused_keys_raise_at_construction_with_the_reason(on_cpu, keys, match):
    conf = _config(**keys)
    with pytest.raises(NotImplementedError, match=match) as e:
        conf.tracker_class(conf)
    assert len(str(e.value)) > len(match) + 20                                 # (a reason, not only the key's name)


@pytest.mark.parametrize("keys,match", [(dict(chain_deltas=()), "deltas"), (dict(chain_deltas=(0,)), "deltas"),
                                        (dict(chain_deltas=(1, 1)), "deltas"), (dict(chain_deltas=(None, 128)), "deltas"),
                                        (dict(chain_vis_thr=1.5), "vis_thr"), (dict(chain_vis_thr=NAN), "vis_thr"),
                                        (dict(chain_unit_cost=-1.0), "unit_cost"), (dict(chain_iters=0), "iters")])
def test_multiflowtracker_validates_the_chain_keys(on_cpu, keys, match):
    conf = _config(**keys)
    with pytest.raises(ValueError, match=match):
        conf.tracker_class(conf)


def test_set_fast_meta_raises(on_cpu):
    conf = _config()
    trk = conf.tracker_class(conf)
    with pytest.raises(NotImplementedError, match="ring"):
        trk.set_fast_meta(SimpleNamespace(estim_H_current2template=np.eye(3)))
    assert not trk.fast_forward


# ---- the state machine ----------------------------------------------------------------------------------------------------------
def test_state_machine(on_cpu, monkeypatch):
    """Stubbed fold, chain_tc and solver: success, a rejected finite H (returned, lost), fewer than 4 kept (previous pose), the
    estimator's AssertionError (previous pose), a non-finite H (previous pose), recovery; N_lost counts the run of lost frames."""
    import torch
    from woft_amd import ops
    from woft_amd.tracker import _Fit
    Hh, Ww, K = 16, 24, 3
    tc_calls = []

    def fold(best, prev, flow, wl, ml, k, vis_thr, unit_cost, first):
        h, w = flow.shape[1:]
        return best or (torch.zeros(2, h, w), torch.zeros(h, w), torch.ones(h, w), torch.zeros(h, w, dtype=torch.int32))

    def chain_tc(flow, cost, vis, sel, tmask_u8, vis_thr, want_w=True, mask_hw=None, out=None):
        n = flow.shape[1] * flow.shape[2]
        tc_calls.append(dict(want_w=want_w, mask_hw=mask_hw, vis_thr=vis_thr, tmask=tmask_u8, out=out))
        hist = torch.zeros(130, dtype=torch.int32)
        hist[0], hist[1], hist[2], hist[5], hist[128], hist[129] = 10, 20, 30, 99, 7, 8
        return torch.zeros(2, n), torch.ones(1, n) if want_w else None, torch.ones(1, n), hist

    monkeypatch.setattr(ops, "flow_chain_fold", fold)
    monkeypatch.setattr(ops, "chain_tc", chain_tc)
    conf = _config(chain_deltas=(None, 1, 2), chain_vis_thr=0.25)
    trk = conf.tracker_class(conf)
    mask = np.zeros((Hh, Ww), np.uint8)
    mask[4:12, 6:18] = 255
    frame = lambda t: np.full((Hh, Ww, 3), t, np.uint8)
    trk.init(frame(0), mask)
    assert trk.flower.pinned is trk.multi._template and trk._sparse_weights is False and not trk.lost
    H = lambda s: np.array([[1, 0, s], [0, 1, -s], [0, 0, 1.0]])
    bad = np.full((3, 3), NAN)
    script = [(_Fit(H=H(1), success=True), 96), (_Fit(H=H(2), success=False), 96), (_Fit(H=np.eye(3), success=False), 3),
              (AssertionError("too few"), 4), (_Fit(H=bad, success=True), 50), (_Fit(H=H(6), success=True), 96),
              (_Fit(H=H(7), success=False), 40)]
    seen = []

    def solve(src_xy, dst_xy, w, grid, frame_hw, src_mask_u8, dst_valid_u8, bounds, judge, vis=None):
        fit, kept = script[len(seen)]
        seen.append(dict(src=src_xy, w=w, grid=grid, frame_hw=frame_hw, mask=src_mask_u8, valid=dst_valid_u8, bounds=bounds,
                         judge=judge, vis=vis))
        trk.n_kept = kept
        if isinstance(fit, Exception):
            raise fit
        return fit
    trk._solve = solve
    #        returned H, lost, N_lost, success, H_global
    want = [(H(1), False, 0, True, H(1)), (H(2), True, 1, False, H(2)), (H(2), True, 2, False, None), (H(2), True, 3, False, None),
            (H(2), True, 4, False, None), (H(6), False, 0, True, H(6)), (H(7), True, 1, False, H(7))]
    for t, (Hw, lost, n_lost, success, Hg) in enumerate(want, 1):
        Hm, meta = trk.track(frame(t))
        assert np.array_equal(Hm, Hw), t
        assert (meta.lost, meta.N_lost, meta.global_H_success) == (lost, n_lost, success) == (trk.lost, trk.N_lost, success), t
        assert (meta.H_global_cur2init is None) if Hg is None else np.array_equal(meta.H_global_cur2init, Hg), t
        assert meta.n_kept == script[t - 1][1] and np.array_equal(trk.prev_H2init, Hw)
        assert meta.chain_hist.dtype == np.int64 and meta.chain_hist.tolist() == [10, 20, 30]
        assert (meta.chain_invalid, meta.chain_occluded) == (7, 8) and type(meta.chain_invalid) is int is type(meta.chain_occluded)
        assert hasattr(meta, "solver_decision") == (t == 1) == hasattr(meta, "precision")
        s, c = seen[-1], tc_calls[-1]
        assert s["grid"] == (Hh, Ww) == tuple(s["frame_hw"]) and s["bounds"] is True and s["judge"] is True and s["valid"] is None
        assert s["mask"] is trk._template_mask_u8 is c["tmask"] and s["vis"] is not None and s["src"] is None and s["w"] is not None
        assert c["want_w"] is True and tuple(c["mask_hw"]) == (Hh, Ww) and c["vis_thr"] == 0.25 and (c["out"] is None) == (t == 1)
    assert np.array_equal(trk.last_good_H2init, H(6))
    assert trk.flower.calls == sum(len(trk.multi.schedule(t)) for t in range(1, len(want) + 1))
    assert "(None, 1, 2)" in trk.solver_decision
    # init() again: the state and the ring start over
    trk.init(frame(0), mask)
    assert not trk.lost and trk.N_lost == 0 and np.array_equal(trk.prev_H2init, np.eye(3)) and trk.multi.frame_index == 0
