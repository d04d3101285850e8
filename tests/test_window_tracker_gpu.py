"""WOFTWindow (search-window tracker) on the GPU against runs of the REFERENCE's own WOFTWindow (tests/golden/
tracker_window_runs.npz, recorded by tools/gen_window_golden.py), with the yardstick of the full-frame tracker's golden test
(tests/test_tracker_gpu.py: box corners within 1 px of the reference's homography -- the reference runs torch CPU fp32 and the
float-bilinear warp stub, this runs split-bf16 MFMA kernels --, last_good_H2init within 1e-2, identical state flags) plus the
boxes, which are integers and must be EQUAL.  Corners are measured on the template mask's box."""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from woft_amd import presets, synth  # noqa: E402
from woft_amd.window import Box  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
BLOCK_TOL = 16          # of a 32 x 32 block's pixel sum (~130 000): a frame regenerated on another CPU may round a few pixels the other way

RUNS = ["win", "lost", "small", "whole", "down"]


def _corners_err(Ha, Hb, mask):
    b = Box.from_mask(mask > 0)
    c = np.array([[b.tl_x, b.tl_y, 1], [b.br_x, b.tl_y, 1], [b.br_x, b.br_y, 1], [b.tl_x, b.br_y, 1.0]]).T
    pa, pb = np.linalg.inv(Ha) @ c, np.linalg.inv(Hb) @ c
    return np.abs(pa[:2] / pa[2] - pb[:2] / pb[2]).max()


def _block_sums(img, block):
    h, w, c = img.shape
    a = img[:h // block * block, :w // block * block].astype(np.int64)
    return a.reshape(h // block, block, w // block, block, c).sum(axis=(1, 3))


def _sequence(g, name):
    """The run's template, mask and frames, regenerated from the recorded synth arguments and checked against the recorded sums."""
    Hh, Ww, seq_id = (int(v) for v in g[f"{name}_synth"])
    template = synth.make_template(Hh, Ww, seq_id=seq_id)
    frames = [synth.make_frame(template, int(t)) for t in g[f"{name}_ts"]]
    block = int(g["block"])
    for img, want in zip([template] + frames, g[f"{name}_sums"]):
        assert np.abs(_block_sums(img, block) - want).max() <= BLOCK_TOL, name
    return template, g[f"{name}_mask"], frames


def _config(g, name, sd, cfg="WOFT_window.py"):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / cfg)
    conf.flow_config.model = sd
    conf.flow_config.iters = int(g["iters"])
    conf.flow_config.padding_mode = "RAFT"
    if cfg == "WOFT_window.py":
        conf.search_window_margin = float(g[f"{name}_margin"]) or None
    if int(g[f"{name}_downscale"]):
        conf.downscale_inputs = int(g[f"{name}_downscale"])
    return conf


def _run(g, name, sd, backend, monkeypatch, host_frames=True, check=True):
    monkeypatch.setenv("WOFT_FUSED", "1" if backend == "device" else "0")
    conf = _config(g, name, sd)
    tracker = conf.tracker_class(conf)
    assert type(tracker).__name__ == "WOFTWindow" and (tracker._fused is not None) == (backend == "device")
    template, mask, frames = _sequence(g, name)
    k = int(g[f"{name}_downscale"]) or 1
    small_mask = mask[::k, ::k]
    tracker.init(template, mask)
    if check:
        assert tracker.search_bbox.as_xywh() == tuple(g[f"{name}_search_box"]), name
    fail = set(int(i) for i in g[f"{name}_force_fail"])
    local = {int(r[0]): tuple(r[1:]) for r in g[f"{name}_local_boxes"]}
    normal, never = conf.redet_success_fn, presets.redetection_by_inliers(1e-6, 0.999)
    S, Sinv = np.diag([1.0 / k, 1.0 / k, 1.0]), np.diag([float(k), float(k), 1.0])
    to_work = lambda Hm: S @ Hm @ Sinv                 # (track() returns the pose at input scale; the meta fields are at working scale)
    results = []
    for i, f in enumerate(frames):
        tracker.C.redet_success_fn = never if i in fail else normal           # config-level hook, as in the golden run
        tracker._fused = tracker._fused_specs()
        Hg, mg = tracker.track(f if host_frames else torch.from_numpy(f).cuda())
        results.append((Hg, mg, tracker.local_search_bbox))
        if not check:
            continue
        lost, n_lost, ok, has_local = g[f"{name}_meta"][i]
        assert (mg.lost, mg.N_lost, bool(mg.global_H_success)) == (bool(lost), int(n_lost), bool(ok)), (name, i)
        errs = [_corners_err(to_work(Hg), to_work(g[f"{name}_H"][i]), small_mask),
                _corners_err(mg.H_global_cur2init, g[f"{name}_Hglobal_{i}"], small_mask)]
        assert hasattr(mg, "H_local_cur2init") == bool(has_local)
        if has_local:
            errs.append(_corners_err(mg.H_local_cur2init, g[f"{name}_Hlocal_{i}"], small_mask))
            assert tracker.local_search_bbox.as_xywh() == local[i], (name, i, tracker.local_search_bbox, local[i])
        else:
            assert tracker.local_search_bbox is None
        print(f"{name}[{backend}] frame {i}: corners within {max(errs):.4f} px of the reference's WOFTWindow")
        assert max(errs) < 1.0, (name, i, errs)
        assert np.allclose(mg.last_good_H2init, g[f"{name}_lastgood_{i}"], atol=1e-2)
    return results


@pytest.mark.parametrize("backend", ["device", "callables"])
@pytest.mark.parametrize("name", RUNS)
def test_window_tracker_vs_reference_window_tracker_runs(golden_dir, monkeypatch, name, backend):
    g = np.load(golden_dir / "tracker_window_runs.npz")
    assert list(g["runs"]) == RUNS
    _run(g, name, synth.make_state_dict(seed=int(g["seed"])), backend, monkeypatch)


@pytest.mark.parametrize("name", ["lost", "small"])
def test_device_back_end_equals_callable_back_end(golden_dir, monkeypatch, name):
    """The margins of tests/test_tracker_gpu.py for this pair (test_fused_path_equals_generic_path): identical."""
    g = np.load(golden_dir / "tracker_window_runs.npz")
    sd = synth.make_state_dict(seed=int(g["seed"]))
    a = _run(g, name, sd, "device", monkeypatch, check=False)
    b = _run(g, name, sd, "callables", monkeypatch, check=False)
    for (Ha, ma, ba), (Hb, mb, bb) in zip(a, b):
        assert ma.lost == mb.lost and ma.N_lost == mb.N_lost and bool(ma.global_H_success) == bool(mb.global_H_success)
        assert np.array_equal(Ha, Hb), np.abs(Ha - Hb).max()
        assert np.array_equal(ma.H_global_cur2init, mb.H_global_cur2init) and ba == bb


def test_numpy_frames_equal_device_frames(golden_dir, monkeypatch):
    g = np.load(golden_dir / "tracker_window_runs.npz")
    sd = synth.make_state_dict(seed=int(g["seed"]))
    a = _run(g, "lost", sd, "device", monkeypatch, host_frames=True, check=False)
    b = _run(g, "lost", sd, "device", monkeypatch, host_frames=False, check=False)
    for (Ha, ma, ba), (Hb, mb, bb) in zip(a, b):
        assert np.array_equal(Ha, Hb) and ma.lost == mb.lost and ba == bb


def _tracker(sd, monkeypatch, cfg="WOFT_window.py", margin=0.25, iters=4, backend="device"):
    from pytracking.utils.config import load_config
    monkeypatch.setenv("WOFT_FUSED", "1" if backend == "device" else "0")
    conf = load_config(ROOT / "pytracking" / "configs" / cfg)
    conf.flow_config.model = sd
    conf.flow_config.iters = iters
    conf.flow_config.padding_mode = "RAFT"
    if cfg == "WOFT_window.py":
        conf.search_window_margin = margin
    return conf, conf.tracker_class(conf)


@pytest.mark.parametrize("backend", ["device", "callables"])
def test_box_at_the_frame_edge_tracks_and_stays_finite(monkeypatch, backend):
    """The deviation: a small mask in the corner, whose minimum-size box the reference would slice with negative indices -- here the
    box is cut to the frame and the tracker runs the sequence, a lost frame included, with finite, invertible poses."""
    Hh, Ww = 256, 320
    sd = synth.make_state_dict(seed=7)
    template = synth.make_template(Hh, Ww, seq_id=11)
    mask = np.zeros((Hh, Ww), np.uint8)
    mask[8:88, 10:110] = 255
    frames = [synth.make_frame(template, t) for t in (1, 2, 3, 4)]
    conf, trk = _tracker(sd, monkeypatch, backend=backend)
    _, full = _tracker(sd, monkeypatch, cfg="WOFT.py", backend=backend)
    trk.init(template, mask)
    full.init(template, mask)
    assert trk.search_bbox.inside(Ww, Hh) and (trk.search_bbox.tl_x, trk.search_bbox.tl_y) == (0, 0)
    assert trk.search_bbox.w < Ww and trk.search_bbox.h < Hh
    normal, never = conf.redet_success_fn, presets.redetection_by_inliers(1e-6, 0.999)
    for i, f in enumerate(frames):
        for t in (trk, full):
            t.C.redet_success_fn = never if i == 2 else normal
            t._fused = t._fused_specs()
        prev_pose = trk.prev_H2init.copy()
        Hw, mw = trk.track(f)
        Hf, mf = full.track(f)
        assert np.all(np.isfinite(Hw)) and np.all(np.isfinite(mw.H_global_cur2init)) and abs(np.linalg.det(Hw)) > 1e-6
        if i == 2:
            assert mw.lost and mf.lost and hasattr(mw, "H_local_cur2init") and np.all(np.isfinite(mw.H_local_cur2init))
            assert trk.local_search_bbox.inside(Ww, Hh)
            # the frame-to-frame flow really ran on the clipped window: its plan exists, and its fit moved the pose
            y0, x0, rows, cols = trk.local_search_bbox.crop_rect()
            assert ((rows + 7) // 8 * 8, (cols + 7) // 8 * 8, 1) in trk.flower.engine._plans
            assert not np.array_equal(mw.H_local_cur2init, prev_pose)
        # (reported, not asserted: the two trackers see different pixels, and the synthetic checkpoint's flow is not a motion estimate)
        print(f"edge box [{backend}] frame {i}: lost {mw.lost} / {mf.lost}; window tracker's box corners "
              f"{_corners_err(Hw, Hf, mask):.3f} px from the full-frame tracker's")


def test_forty_lost_frames_with_a_drifting_box_keep_the_plans_bounded(monkeypatch):
    Hh, Ww = 256, 320
    sd = synth.make_state_dict(seed=7)
    template = synth.make_template(Hh, Ww, seq_id=12)
    mask = np.zeros((Hh, Ww), np.uint8)
    mask[60:160, 60:180] = 255
    conf, trk = _tracker(sd, monkeypatch, iters=2)
    conf.redet_success_fn = presets.redetection_by_inliers(1e-6, 0.999)        # never re-detected: every frame is a lost frame
    trk._fused = trk._fused_specs()
    trk.init(template, mask)
    shapes, peak, first_key = set(), 0, None
    pose = lambda t: np.array([[1.0 + 0.008 * t, 0, 1.0 * t], [0, 1.0 + 0.008 * t, 0.5 * t], [0, 0, 1.0]])   # template -> frame t
    for t in range(1, 41):
        # the object grows and drifts; the previous pose is SET to the sequence's (the synthetic checkpoint's flow follows no motion),
        # so the carried mask, and with it the local window, has a different size nearly every frame
        trk.prev_H2init = np.linalg.inv(pose(t - 1))
        frame = np.ascontiguousarray(np.clip(np.round(synth.warp_image_np(template, pose(t))), 0, 255).astype(np.uint8))
        Hc, m = trk.track(frame)
        assert m.lost and np.all(np.isfinite(Hc)) and hasattr(m, "H_local_cur2init")
        assert not np.array_equal(m.H_local_cur2init, np.linalg.inv(pose(t - 1)))      # the local fit ran and moved the pose
        y0, x0, rows, cols = trk.local_search_bbox.crop_rect()
        assert trk.local_search_bbox.inside(Ww, Hh)
        key = ((rows + 7) // 8 * 8, (cols + 7) // 8 * 8, 1)
        assert key in trk.flower.engine._plans                                     # this frame's local flow has its plan
        first_key = first_key if t > 1 else key
        shapes.add(key)
        peak = max(peak, len(trk.flower.engine._plans))
    assert len(shapes) > trk.PLAN_BOUND + 2, shapes                            # (the sequence does what it is meant to do)
    assert peak == trk.PLAN_BOUND + 1, (peak, sorted(trk.flower.engine._plans))     # the pinned global window + the bound, reached
    assert first_key not in trk.flower.engine._plans and key in trk.flower.engine._plans     # eviction happened: oldest gone, newest kept
    assert len(trk.flower._out) <= trk.PLAN_BOUND + 1 and len(trk._buffers) <= trk.PLAN_BOUND + 1
    assert (trk._rect[2] + 7) // 8 * 8 in [k[0] for k in trk.flower.engine._plans if len(k) == 2]     # the global plan survived


def test_local_window_without_room_keeps_the_previous_pose(monkeypatch):
    """A local window whose crop has a side under MIN_FLOW_SIDE runs no flow and keeps the previous pose.  With the 160-pixel minimum
    size only frames under about a hundred pixels a side get there, so the threshold is raised on the instance to take the branch."""
    Hh, Ww = 256, 320
    sd = synth.make_state_dict(seed=7)
    template = synth.make_template(Hh, Ww, seq_id=14)
    conf, trk = _tracker(sd, monkeypatch)
    conf.redet_success_fn = presets.redetection_by_inliers(1e-6, 0.999)
    trk._fused = trk._fused_specs()
    trk.init(template, synth.make_init_mask(Hh, Ww))
    H1, m1 = trk.track(synth.make_frame(template, 1))                          # an ordinary lost frame: the local flow runs
    assert m1.lost and any(len(k) == 3 for k in trk.flower.engine._plans) and not np.array_equal(m1.H_local_cur2init, np.eye(3))
    plans = set(trk.flower.engine._plans)
    trk.MIN_FLOW_SIDE = 10 ** 6
    prev = trk.prev_H2init.copy()
    H2, m2 = trk.track(synth.make_frame(template, 2))
    assert m2.lost and np.array_equal(m2.H_local_cur2init, prev) and np.array_equal(H2, prev)
    assert trk.local_search_bbox is not None and set(trk.flower.engine._plans) == plans


def test_whole_frame_window_agrees_with_the_full_frame_tracker(monkeypatch):
    """margin falsy: the window is the frame less its last row and column (the reference's exclusive crop) -- same poses as
    YAOFTrackerSingleControl to the corner margin, not bit for bit."""
    Hh, Ww = 256, 320
    sd = synth.make_state_dict(seed=7)
    template = synth.make_template(Hh, Ww, seq_id=13)
    mask = synth.make_init_mask(Hh, Ww)
    _, win = _tracker(sd, monkeypatch, margin=None)
    _, full = _tracker(sd, monkeypatch, cfg="WOFT.py")
    win.init(template, mask)
    full.init(template, mask)
    assert win.search_bbox.as_xywh() == (0, 0, Ww, Hh) and win._rect == (0, 0, Hh - 1, Ww - 1)
    for t in (1, 2, 3, 4):
        f = synth.make_frame(template, t)
        Hw, mw = win.track(f)
        Hf, mf = full.track(f)
        assert (mw.lost, mw.N_lost, bool(mw.global_H_success)) == (mf.lost, mf.N_lost, bool(mf.global_H_success))
        assert _corners_err(Hw, Hf, mask) < 1.0
