"""The photometric refinement inside the tracker (config key `photo_refine`): with the global stage replaced
by a stub that reports a known perturbed pose, track() must return exactly what woft_amd.photo.refine_homography makes of that
pose, keep the un-refined pose in meta.H_flow_cur2init, leave lost frames alone, be byte-identical to WOFT with the key at 0,
be refused by the chained trackers and reject bad values at construction."""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import photo_host as ph  # noqa: E402
from woft_amd import hsynth, photo, synth  # noqa: E402
from woft_amd.homography import compose_H  # noqa: E402
from woft_amd.planar import _Fit  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
HW = (128, 160)


def _config(name="WOFT_photo.py", **keys):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / name)
    conf.flow_config.model = synth.make_state_dict(seed=7)
    conf.flow_config.iters = 3
    for k, v in keys.items():
        setattr(conf, k, v)
    return conf


@pytest.fixture(scope="module")
def scene():
    """Template, mask, a frame under a known H_gt with gain and bias, and the perturbed pose the stub reports (frame -> template)."""
    rs = np.random.RandomState(31)
    template, mask = synth.make_template(HW[0], HW[1], seq_id=5), synth.make_init_mask(*HW)
    c = ph.box_corners((40, 32, 119, 95))
    H_gt = hsynth.homography_from_4pts(c, c + rs.uniform(-4.0, 4.0, (4, 2)))
    frame = ph.render_frame(template, H_gt, out_hw=HW)
    W0 = hsynth.homography_from_4pts(c, ph.project(H_gt, c) + rs.uniform(-1.5, 1.5, (4, 2)))
    return template, mask, frame, H_gt, compose_H(np.linalg.inv(W0))


def _stub(tracker, H, success=True):
    tracker._global_stage = lambda frame, prewarp_H: _Fit(H=H.copy(), success=success)


@pytest.mark.parametrize("cfg", ["WOFT_photo.py", "WOFT_window.py"])
def test_track_returns_the_refined_pose(scene, cfg):
    template, mask, frame, H_gt, H_flow = scene
    conf = _config(cfg, photo_refine=10)
    tracker = conf.tracker_class(conf)
    assert "photometric refinement" in tracker.solver_decision
    tracker.init(template, mask)
    _stub(tracker, H_flow)
    H, meta = tracker.track(frame)
    W, info = photo.refine_homography(template, mask, frame, np.linalg.inv(H_flow), iters=10)
    want = compose_H(np.linalg.inv(W))
    assert info.best >= 0 and np.array_equal(H, want)
    assert np.array_equal(tracker.prev_H2init, want) and np.array_equal(tracker.last_good_H2init, want)
    assert np.array_equal(meta.H_flow_cur2init, H_flow) and not meta.lost
    p = meta.photo
    assert (p.status, p.best, p.iterates) == (info.status, info.best, len(info.cost))
    assert (p.rms_before, p.rms_after, p.n_valid) == (info.rms_before, info.rms_after, int(info.n_valid[info.best]))
    assert (p.gain, p.bias) == (float(info.gain[info.best]), float(info.bias[info.best])) and p.rms_after <= p.rms_before
    c = ph.box_corners((40, 32, 119, 95))
    err = lambda Hc: float(np.sqrt(((ph.project(np.linalg.inv(Hc), c) - ph.project(H_gt, c)) ** 2).sum(1)).max())
    print(f"{cfg}: corner error against H_gt {err(H_flow):.3f} -> {err(H):.3f} px, {p.status} after {p.iterates} iterates, "
          f"cost {p.rms_before:.2f} -> {p.rms_after:.2f}")
    assert err(H) < err(H_flow)


def test_blurred_inputs(scene):
    template, mask, frame, _, H_flow = scene
    conf = _config(photo_refine=4, photo_blur_sigma=1.0, photo_huber_k=6.0, photo_stride=2)
    tracker = conf.tracker_class(conf)
    tracker.init(template, mask)
    _stub(tracker, H_flow)
    H, meta = tracker.track(frame)
    blur = lambda a: hsynth.augment(torch.from_numpy(a).cuda(), blur_sigma=1.0, want_f32=True)[1]
    W, info = photo.refine_homography(blur(template), mask, blur(frame), np.linalg.inv(H_flow), iters=4, huber_k=6.0, stride=2)
    assert info.best >= 0 and np.array_equal(H, compose_H(np.linalg.inv(W))) and meta.photo.iterates == len(info.cost)


def test_downscaled_inputs_are_refined_at_the_working_scale(scene):
    """`downscale_inputs`: the stage runs on the downscaled images the tracker holds; track() returns the pose at input scale."""
    from woft_amd import ops
    template, mask, frame, _, H_flow = scene
    conf = _config("WOFT_downscale_2x.py", photo_refine=5)
    tracker = conf.tracker_class(conf)
    tracker.init(template, mask)
    S, Sinv = np.diag([0.5, 0.5, 1.0]), np.diag([2.0, 2.0, 1.0])
    H_small = compose_H(Sinv, H_flow, S)                              # the stub's pose, at the working scale
    _stub(tracker, H_small)
    H, meta = tracker.track(frame)
    small = lambda a: ops.resize_by_factor_u8(torch.from_numpy(a).cuda(), 2)
    W, info = photo.refine_homography(small(template), small(mask), small(frame), np.linalg.inv(H_small), iters=5)
    want = compose_H(np.linalg.inv(W))
    assert info.best >= 0 and np.array_equal(tracker.prev_H2init, want) and np.array_equal(H, compose_H(S, want, Sinv))
    assert np.array_equal(meta.H_flow_cur2init, H_small) and meta.photo.n_valid == int(info.n_valid[info.best])


def test_lost_frame_is_not_refined(scene):
    template, mask, frame, _, H_flow = scene
    conf = _config(no_local_H=True)
    tracker = conf.tracker_class(conf)
    tracker.init(template, mask)
    _stub(tracker, H_flow, success=False)
    H, meta = tracker.track(frame)
    assert meta.lost and np.array_equal(H, H_flow) and not hasattr(meta, "photo") and not hasattr(meta, "H_flow_cur2init")
    assert np.array_equal(tracker.prev_H2init, H_flow) and np.array_equal(tracker.last_good_H2init, np.eye(3))


def test_zero_iterations_is_woft(scene):
    template, mask = scene[0], scene[1]
    frames = [synth.make_frame(template, t) for t in (1, 2, 3)]
    runs = []
    for conf in (_config("WOFT.py"), _config(photo_refine=0)):
        tracker = conf.tracker_class(conf)
        assert tracker._photo is None and "photometric" not in tracker.solver_decision
        tracker.init(template, mask)
        out = [tracker.track(f) for f in frames]
        assert all(not hasattr(m, "photo") for _, m in out)
        runs.append(b"".join(np.ascontiguousarray(H).tobytes() for H, _ in out))
    assert runs[0] == runs[1]


def test_headless_demo_runs_the_config_unchanged(scene, tmp_path):
    import sys
    from PIL import Image
    sys.path.insert(0, str(ROOT / "tools"))
    import woft_demo_headless as demo
    template = scene[0]
    frames = [template] + [synth.make_frame(template, t) for t in (1, 2)]
    src = tmp_path / "frames"
    src.mkdir()
    for i, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(src / f"{i:04d}.png")
    roi = (HW[1] // 4, HW[0] // 4, HW[1] // 2 - 1, HW[0] // 2 - 1)
    res = demo.run(src, ROOT / "pytracking" / "configs" / "WOFT_photo.py", roi, weights="synthetic:7", iters=3)
    assert len(res) == 2 and all(m is not None for _, m in res)
    conf = _config()
    trk = conf.tracker_class(conf)
    trk.init(template, demo.rect_mask(template, *roi))
    for (Hd, md), f in zip(res, frames[1:]):
        Ht, mt = trk.track(f)
        assert np.array_equal(Hd, Ht) and md.lost == mt.lost and hasattr(md, "photo") == (not md.lost)


def test_chained_trackers_refuse_the_key():
    for cfg in ("WOFT_chained.py", "WOFT_chained_window.py", "WOFT_chained_multi.py"):
        conf = _config(cfg, photo_refine=10)
        with pytest.raises(NotImplementedError, match="photo_refine"):
            conf.tracker_class(conf)


@pytest.mark.parametrize("keys", [dict(photo_refine=-1), dict(photo_refine=2.5), dict(photo_refine="ten"), dict(photo_refine=True),
                                  dict(photo_refine=65), dict(photo_huber_k=0.0), dict(photo_stride=0), dict(photo_stride=1.5),
                                  dict(photo_min_valid=2.0), dict(photo_eps=-1.0), dict(photo_blur_sigma=-1.0),
                                  dict(photo_blur_sigma=float("nan"))])
def test_bad_values_raise(keys):
    conf = _config(**keys)
    with pytest.raises(ValueError):
        conf.tracker_class(conf)
