"""Several planar targets on one chained flow, on the host: the three new entry points in the header, EXPORTS
and the library, their argument checks (the error code before any device work), the bit-plane packing, init()'s input validation,
WOFTChained's refusals, and the shipped config."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = ("woft_chain_tc_multi", "woft_tc_select_multi", "woft_tc_select_multi_ws_bytes", "woft_inlier_frac_batched")


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_exports_and_library_agree_on_the_new_names(lib):
    from woft_amd import _lib, ops
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name), name
    assert [len(_lib._SIGS[n][1]) for n in NEW] == [16, 21, 2, 9]
    assert re.search(r"^#define\s+WOFT_MULTI_MAX_TARGETS\s+32\s*$", header, flags=re.M) and ops.MULTI_MAX_TARGETS == 32
    assert all(hasattr(ops, n) for n in ("chain_tc_multi", "tc_select_multi", "tc_select_multi_ws", "inlier_frac_batched"))


def _buffers(n_slots, slot_bytes=4096):
    buf = (ctypes.c_uint8 * (n_slots * slot_bytes))()
    base = ctypes.addressof(buf)
    return buf, (lambda j: base + slot_bytes * j)


def test_chain_tc_multi_rejects_bad_arguments_without_a_device(lib):
    """-1 before any launch (host buffers stand in for device ones: nothing is dereferenced; only refused calls are made)."""
    gh, gw, mh, mw, K = 5, 7, 6, 9, 3
    keep, at = _buffers(10)
    good = dict(flow=at(0), cost=at(1), vis=at(2), sel=at(3), tbits=at(4), gh=gh, gw=gw, mh=mh, mw=mw, n_targets=K, vis_thr=0.5,
                dst=at(5), w=at(6), ok=at(7), hist=at(8))
    order = list(good)
    call = lambda **kw: lib.woft_chain_tc_multi(*[dict(good, **kw)[n] for n in order], None)
    plane = 4 * gh * gw
    bad = [dict(flow=None), dict(cost=None), dict(vis=None), dict(sel=None), dict(tbits=None), dict(dst=None), dict(ok=None),
           dict(hist=None), dict(n_targets=0), dict(n_targets=33), dict(n_targets=-1), dict(gh=0), dict(gw=-2),
           dict(gh=(1 << 24) + 1), dict(mh=gh - 1), dict(mw=gw - 1), dict(vis_thr=-0.1), dict(vis_thr=1.5), dict(vis_thr=float("nan")),
           # an output on an input, at its last byte, and on another output; the histogram is K rows long
           dict(dst=good["flow"]), dict(ok=good["tbits"] + 4 * mh * mw - 1), dict(w=good["dst"] + plane), dict(hist=good["sel"]),
           dict(hist=good["ok"] - 4 * 130 * K + 1), dict(hist=good["dst"] + 2 * plane - 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    del keep


def test_tc_select_multi_rejects_bad_arguments_without_a_device(lib):
    gh, gw, mh, mw, K, cap = 5, 7, 6, 9, 3, 16
    n = gh * gw
    ws_bytes = lib.woft_tc_select_multi_ws_bytes(n, K)
    # per target 4 + 2 * nb + 1024 int32, rounded up to 16 bytes, then one uint32 of keep bits per pixel (n rounded up to 4)
    assert ws_bytes == ((K * (4 + 2 * 1 + 1024) + 3) // 4 * 4 + (n + 3) // 4 * 4) * 4
    assert lib.woft_tc_select_multi_ws_bytes(1920 * 1080, 32) == ((32 * (4 + 2 * 2025 + 1024) + 3) // 4 * 4 + 1920 * 1080) * 4
    for a in ((n, 0), (n, 33), (-1, 3)):
        assert lib.woft_tc_select_multi_ws_bytes(*a) == -1
    keep, at = _buffers(12, slot_bytes=16384)
    good = dict(dst=at(0), w=at(1), tbits=at(2), gh=gh, gw=gw, mh=mh, mw=mw, n_targets=K, check_dst=1, sobol_u=at(3), n_draw=8,
                vis=at(4), vis_mode=1, vis_thr=0.5, ws=at(5), pa=at(6), pb=at(7), wout=at(8), cap=cap, count=at(9))
    assert ws_bytes <= 16384
    order = list(good)
    call = lambda **kw: lib.woft_tc_select_multi(*[dict(good, **kw)[n] for n in order], None)
    bad = [dict(dst=None), dict(tbits=None), dict(ws=None), dict(pa=None), dict(pb=None), dict(count=None),
           dict(n_targets=0), dict(n_targets=33), dict(gh=0), dict(gw=0), dict(mh=gh - 1), dict(mw=gw - 1), dict(cap=0),
           dict(n_draw=-1), dict(n_draw=1025), dict(sobol_u=None), dict(vis_mode=3), dict(vis_mode=-1), dict(vis_thr=float("nan")),
           dict(gh=1 << 16, gw=1 << 15, mh=1 << 16, mw=1 << 15),
           dict(pa=good["dst"]), dict(pb=good["dst"] + 8 * n - 1), dict(wout=good["w"]), dict(count=good["vis"] + 4 * n - 1),
           dict(ws=good["tbits"]), dict(pa=good["sobol_u"]), dict(pb=good["pa"] + 8 * K * cap - 1), dict(count=good["wout"]),
           dict(wout=good["ws"] + ws_bytes - 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    del keep


def test_inlier_frac_batched_rejects_bad_arguments_without_a_device(lib):
    B, n = 4, 10
    keep, at = _buffers(6)
    good = dict(pa=at(0), pb=at(1), batch=B, n_max=n, counts=at(2), H=at(3), thr=5.0, frac=at(4))
    order = list(good)
    call = lambda **kw: lib.woft_inlier_frac_batched(*[dict(good, **kw)[k] for k in order], None)
    bad = [dict(pa=None), dict(pb=None), dict(H=None), dict(frac=None), dict(batch=0), dict(batch=-3), dict(batch=65536),
           dict(n_max=-1), dict(frac=good["pa"]), dict(frac=good["pb"] + 8 * B * n - 1), dict(frac=good["H"] + 36 * B - 1),
           dict(frac=good["counts"]), dict(frac=good["H"] - 4 * B + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    del keep


def test_bit_plane_packing():
    from woft_amd import pack_target_bits
    a = np.zeros((4, 5), np.uint8)
    b = np.zeros((4, 5), bool)
    c = np.zeros((4, 5), np.uint8)
    a[1:3, 1:4] = 255
    b[2:4, 3:5] = True                                                          # (overlaps a at (2, 3))
    bits = pack_target_bits([a, b, c])
    assert bits.dtype == np.uint32 and bits.shape == (4, 5)
    for t, m in enumerate((a, b, c)):
        assert np.array_equal((bits >> t) & 1, (m != 0).astype(np.uint32))
    assert bits[2, 3] == 3 and bits[1, 1] == 1 and bits[3, 4] == 2 and bits[0, 0] == 0
    full = pack_target_bits([np.ones((2, 3), np.uint8)] * 32)
    assert (full == 0xFFFFFFFF).all() and (full.view(np.int32) == -1).all()     # (bit 31 survives the int32 view the device reads)
    for bad in ([], [a] * 33, [a, np.zeros((4, 6), np.uint8)]):
        with pytest.raises(ValueError):
            pack_target_bits(bad)


# ---- the tracker's construction and init() ----------------------------------------------------------------------------------------
class _StubProvider:
    def __init__(self, cfg):
        self.C = cfg

    def pin_source(self, img):
        self.pinned = img


@pytest.fixture
def on_cpu(monkeypatch):
    from woft_amd import multiflow, tracker
    monkeypatch.setattr(tracker.YAOFTrackerSingleControl, "DEVICE", "cpu")
    monkeypatch.setattr(multiflow.MultiFlowTracker, "DEVICE", "cpu")
    monkeypatch.delenv("WOFT_FUSED", raising=False)


def _config(**keys):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained_multi.py")
    conf.flow_config.of_class = _StubProvider
    for k, v in keys.items():
        setattr(conf, k, v)
    return conf


def test_shipped_config_and_exports():
    import woft_amd
    from pytracking.tracker.WOFT_chained import WOFTChained, WOFTChainedMulti
    from pytracking.utils.config import load_config
    from woft_amd import chained
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained_multi.py")
    single = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained.py")
    assert conf.tracker_class is WOFTChainedMulti is chained.WOFTChainedMulti is woft_amd.WOFTChainedMulti
    assert issubclass(WOFTChainedMulti, WOFTChained) and single.tracker_class is WOFTChained
    assert woft_amd.pack_target_bits is chained.pack_target_bits
    for k in ("chain_deltas", "chain_vis_thr", "chain_unit_cost", "chain_iters", "chain_weights"):
        assert getattr(conf, k) == getattr(single, k), k


def test_routes_and_solver_decision(on_cpu, monkeypatch):
    from woft_amd import presets
    from woft_amd.chained import WOFTChained
    conf = _config()
    trk = conf.tracker_class(conf)
    one = WOFTChained(_config())
    assert trk._route == "batched" and trk.solver_decision.startswith(one.solver_decision + "; multi-target planar stage")
    assert trk._decision_for_meta() == one.solver_decision and "one batched fit" in trk.solver_decision
    for est, word in ((presets.estimator_ransac(), "RANSAC"), (presets.estimator_trs(), "TRS")):
        trk = _config(H_estimator=est)
        trk = trk.tracker_class(trk)
        assert trk._route == "select" and word in trk.solver_decision
    trk = _config(subsampler_fn=None)
    trk = trk.tracker_class(trk)
    assert trk._fused is not None and trk._route == "loop" and "no subsampler" in trk.solver_decision
    trk = _config(device_solver=False)
    trk = trk.tracker_class(trk)
    assert trk._fused is None and trk._route == "loop" and "callables" in trk.solver_decision


def test_init_validates_the_masks(on_cpu):
    conf = _config()
    trk = conf.tracker_class(conf)
    frame = np.zeros((16, 24, 3), np.uint8)
    mask = np.zeros((16, 24), np.uint8)
    mask[4:12, 6:18] = 255
    with pytest.raises(RuntimeError, match="before init"):
        trk.track(frame)
    for bad in ([], [mask] * 33, np.zeros((0, 16, 24), np.uint8)):
        with pytest.raises(ValueError, match="1 to 32"):
            trk.init(frame, bad)
    with pytest.raises(ValueError, match="target 1.*shape"):
        trk.init(frame, [mask, mask[:, :-1]])
    with pytest.raises(ValueError, match="target 0.*dtype"):
        trk.init(frame, [mask.astype(np.float32)])
    with pytest.raises(ValueError, match="target 1.*dtype"):
        trk.init(frame, [mask, mask.astype(np.int64)])
    with pytest.raises(ValueError, match="K, H, W"):
        trk.init(frame, mask)                                                   # (a single (H, W) array is not a list of masks)
    two = mask.copy()
    two[0:2, 0:2] = 255
    with pytest.raises(AssertionError, match="target 2"):
        trk.init(frame, [mask, mask > 0, two])
    assert trk._targets == []                                                   # (a refused init leaves no half-built state)
    trk.init(frame, np.stack([mask, mask]) > 0)
    assert len(trk._targets) == 2 and trk._tbits.shape == (16, 24) and int(trk._tbits[5, 7]) == 3
    assert all(not T.lost and T.N_lost == 0 and np.array_equal(T.prev_H2init, np.eye(3)) for T in trk._targets)
    assert trk._targets[0].prev_H2init is not trk._targets[1].prev_H2init


@pytest.mark.parametrize("keys,match", [
    (dict(visibility_mode="gate"), "visibility_mode"), (dict(fb_check="gate"), "fb_check"),
    (dict(warm_start_local=True), "warm_start_local"), (dict(downscale_inputs=2), "downscale_inputs"),
    (dict(search_window_margin=0.25), "search_window_margin"),
    (dict(post_hoc_weights_postprocessing_fn=lambda w: w), "post_hoc_weights_postprocessing_fn")])
def test_the_refusals_of_the_single_target_tracker_hold(on_cpu, keys, match):
    conf = _config(**keys)
    with pytest.raises(NotImplementedError, match=match):
        conf.tracker_class(conf)


def test_set_fast_meta_is_refused(on_cpu):
    conf = _config()
    trk = conf.tracker_class(conf)
    with pytest.raises(NotImplementedError, match="ring"):
        trk.set_fast_meta(object())
