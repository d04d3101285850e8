"""The photometric refinement inside the chained trackers (config key `chain_photo_refine`) on the stub
provider of tests/chained_multi_util.py with textured frames: with the fit stubbed to a known perturbed pose, track() returns what
woft_amd.photo.refine_homography makes of that pose; the multi-target trackers return, target by target, the bytes of K
single-target trackers with the key on every route; a lost target is left alone; the key at 0 is the key absent; bad values are
refused at construction; and the batched routes make one woft_photo_refine_multi call per frame whatever K."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import chained_multi_util as U  # noqa: E402
import photo_host as ph  # noqa: E402
from woft_amd import _lib, hsynth, photo, presets, synth  # noqa: E402
from woft_amd.homography import compose_H  # noqa: E402
from woft_amd.planar import _Fit  # noqa: E402

BOX = (16, 12, 47, 35)                 # stub_masks()[0]'s box


@pytest.fixture(scope="module")
def frames():
    """Frame 0 (the template) and frames 1 .. S_FRAMES: a synthetic texture rendered under motion(t); pixel (0, 0), outside every
    mask, holds the frame index AffineProvider reads."""
    template = synth.make_template(U.SH, U.SW, seq_id=4)
    out = [template.copy()] + [ph.render_frame(template, U.motion(t), gain=1.0, bias=0.0, out_hw=(U.SH, U.SW))
                               for t in range(1, U.S_FRAMES + 1)]
    for t, f in enumerate(out):
        f[0, 0, :] = t
    return out


def _config(name, estimator=None, **keys):
    from pytracking.utils.config import load_config
    conf = load_config(U.ROOT / "pytracking" / "configs" / name)
    conf.flow_config.raft_type = "weighted"
    conf.flow_config.of_class = lambda fc: U.AffineProvider(fc, None)
    conf.chain_deltas = U.S_DELTAS
    if estimator is not None:
        conf.H_estimator = estimator
    for k, v in keys.items():
        setattr(conf, k, v)
    return conf


def _tracker(name, **keys):
    conf = _config(name, **keys)
    return conf.tracker_class(conf)


def _corner_error(H_cur2init, t):
    c = ph.box_corners(BOX)
    return float(np.sqrt(((ph.project(np.linalg.inv(H_cur2init), c) - ph.project(U.motion(t), c)) ** 2).sum(1)).max())


# ---- 1. the single-target trackers on a stubbed fit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["WOFT_chained.py", "WOFT_chained_window.py"])
def test_track_returns_the_refined_pose(frames, cfg):
    t, mask = 1, U.stub_masks()[0]
    c = ph.box_corners(BOX)
    W0 = hsynth.homography_from_4pts(c, ph.project(U.motion(t), c) + np.random.RandomState(31).uniform(-1.5, 1.5, (4, 2)))
    H_flow = compose_H(np.linalg.inv(W0))
    keys = dict(chain_prewarp=False) if "window" in cfg else {}
    trk = _tracker(cfg, chain_photo_refine=6, **keys)
    assert "photometric refinement" in trk.solver_decision
    trk.init(frames[0], mask)

    def fit(*a, **k):
        trk.n_kept = 100
        return _Fit(H=H_flow.copy(), success=True)
    trk._solve = fit
    H, meta = trk.track(frames[t])
    W, info = photo.refine_homography(frames[0], mask, frames[t], np.linalg.inv(H_flow), iters=6)
    want = compose_H(np.linalg.inv(W))
    assert info.best >= 0 and np.array_equal(H, want)
    assert np.array_equal(trk.prev_H2init, want) and np.array_equal(trk.last_good_H2init, want)
    assert np.array_equal(meta.H_flow_cur2init, H_flow) and np.array_equal(meta.H_global_cur2init, H_flow) and not meta.lost
    p = meta.photo
    assert (p.status, p.best, p.iterates) == (info.status, info.best, len(info.cost))
    assert (p.rms_before, p.rms_after, p.n_valid) == (info.rms_before, info.rms_after, int(info.n_valid[info.best]))
    assert (p.gain, p.bias) == (float(info.gain[info.best]), float(info.bias[info.best])) and p.rms_after <= p.rms_before
    print(f"{cfg}: corner error against the motion {_corner_error(H_flow, t):.3f} -> {_corner_error(H, t):.3f} px, {p.status} after "
          f"{p.iterates} iterates, cost {p.rms_before:.2f} -> {p.rms_after:.2f}")
    assert _corner_error(H, t) < _corner_error(H_flow, t)


def test_options_reach_the_refinement(frames):
    mask = U.stub_masks()[0]
    trk = _tracker("WOFT_chained.py", chain_photo_refine=4, chain_photo_blur_sigma=1.0, chain_photo_huber_k=6.0, chain_photo_stride=2,
                   chain_photo_gain_bias=False, chain_photo_eps=0.0, chain_photo_min_valid=0.25)
    trk.init(frames[0], mask)
    H, meta = trk.track(frames[1])
    assert not meta.lost
    blur = lambda a: hsynth.augment(torch.from_numpy(a).cuda(), blur_sigma=1.0, want_f32=True)[1]
    W, info = photo.refine_homography(blur(frames[0]), mask, blur(frames[1]), np.linalg.inv(meta.H_flow_cur2init), iters=4, huber_k=6.0,
                                      stride=2, gain_bias=False, eps=0.0, min_valid=0.25)
    assert info.best >= 0 and np.array_equal(H, compose_H(np.linalg.inv(W))) and meta.photo.iterates == len(info.cost) == 5


# ---- 2. the multi-target trackers against single-target trackers, every route ----------------------------------------------------------
def _multi_and_singles(frames, multi_cfg, single_cfg, masks, **keys):
    trk = _tracker(multi_cfg, **keys)
    trk.init(frames[0], masks)
    multi = [trk.track(f) for f in frames[1:]]
    singles = []
    for m in masks:
        one = _tracker(single_cfg, **keys)
        one.init(frames[0], m)
        singles.append([one.track(f) for f in frames[1:]])
    return trk, multi, singles


def _check_refined(multi, n_targets=3):
    for f, (Hs, metas) in enumerate(multi, 1):
        for k in range(n_targets):
            if k == 2:          # the 1 x 3 target: lost on every frame, never refined
                assert metas[k].lost and not hasattr(metas[k], "photo") and not hasattr(metas[k], "H_flow_cur2init")
                assert np.array_equal(Hs[k], np.eye(3))
            else:
                assert not metas[k].lost and metas[k].photo is not None
                assert np.array_equal(metas[k].H_flow_cur2init, metas[k].H_global_cur2init)


@pytest.mark.parametrize("route", ["batched", "select", "loop"])
def test_multi_equals_single_trackers(monkeypatch, frames, route):
    monkeypatch.setenv("WOFT_FUSED", "0" if route == "loop" else "1")
    keys = dict(chain_photo_refine=6)
    if route == "select":
        keys["estimator"] = presets.estimator_ransac(10000, 3.0, 0.995)
    trk, multi, singles = _multi_and_singles(frames, "WOFT_chained_multi.py", "WOFT_chained.py", U.stub_masks(), **keys)
    assert trk._route == route and "photometric refinement" in trk.solver_decision
    U.assert_same_result(multi, singles, route)
    _check_refined(multi)
    errs = [(_corner_error(m[0].H_flow_cur2init, f), _corner_error(Hs[0], f)) for f, (Hs, m) in enumerate(multi, 1)]
    print(f"{route}: corner error of target 0 per frame, fit -> refined: " + ", ".join(f"{a:.3f} -> {b:.3f}" for a, b in errs))


def test_multi_window_equals_the_window_tracker(monkeypatch, frames):
    monkeypatch.setenv("WOFT_FUSED", "1")
    mask = U.stub_masks()[0]
    trk, multi, singles = _multi_and_singles(frames, "WOFT_chained_multi_window.py", "WOFT_chained_window.py", [mask],
                                             chain_photo_refine=6, chain_prewarp=False)
    assert trk._route == "batched"
    U.assert_same_result(multi, singles, "window")
    assert all(not m[0].lost and m[0].photo is not None and hasattr(m[0], "chain_window") for _, m in multi)


# ---- 3. a lost target ------------------------------------------------------------------------------------------------------------------
def test_lost_frame_is_not_refined(frames):
    mask = U.stub_masks()[0]
    trk = _tracker("WOFT_chained.py", chain_photo_refine=6)
    trk.init(frames[0], mask)
    H_flow = np.linalg.inv(U.motion(1))

    def fit(*a, **k):
        trk.n_kept = 100
        return _Fit(H=H_flow.copy(), success=False)
    trk._solve = fit
    H, meta = trk.track(frames[1])
    assert meta.lost and np.array_equal(H, H_flow) and not hasattr(meta, "photo") and not hasattr(meta, "H_flow_cur2init")
    assert np.array_equal(trk.prev_H2init, H_flow) and np.array_equal(trk.last_good_H2init, np.eye(3))


# ---- 4. the key absent is the key at 0 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["WOFT_chained.py", "WOFT_chained_window.py", "WOFT_chained_multi.py", "WOFT_chained_multi_window.py"])
def test_key_absent_is_key_zero(monkeypatch, frames, cfg):
    monkeypatch.setenv("WOFT_FUSED", "1")
    multi = "multi" in cfg
    keys = dict(chain_prewarp=False) if "window" in cfg else {}
    runs = []
    for extra in ({}, dict(chain_photo_refine=0), dict(chain_photo_refine=None)):
        trk = _tracker(cfg, **keys, **extra)
        assert trk._photo is None and "photometric" not in trk.solver_decision
        trk.init(frames[0], U.stub_masks() if multi else U.stub_masks()[0])
        out = [trk.track(f) for f in frames[1:4]]
        for _, m in out:
            assert all(not hasattr(x, "photo") and not hasattr(x, "H_flow_cur2init") for x in (m if multi else [m]))
        runs.append(out if multi else [(H[None], [m]) for H, m in out])
    for other in runs[1:]:
        K = len(runs[0][0][1])
        U.assert_same_result(other, [[(Hs[k], metas[k]) for Hs, metas in runs[0]] for k in range(K)], cfg)


# ---- 5. bad values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", [dict(chain_photo_refine=-1), dict(chain_photo_refine=2.5), dict(chain_photo_refine="ten"),
                                  dict(chain_photo_refine=True), dict(chain_photo_refine=65), dict(chain_photo_huber_k=0.0),
                                  dict(chain_photo_stride=0), dict(chain_photo_stride=1.5), dict(chain_photo_min_valid=2.0),
                                  dict(chain_photo_eps=-1.0), dict(chain_photo_blur_sigma=-1.0),
                                  dict(chain_photo_blur_sigma=float("nan"))])
def test_bad_values_raise(keys):
    for cfg in ("WOFT_chained_photo.py", "WOFT_chained_multi_photo.py"):
        with pytest.raises(ValueError, match="chain_photo_"):
            _tracker(cfg, **keys)


def test_the_photo_configs_are_the_base_configs_plus_the_key():
    for cfg, cls in (("WOFT_chained_photo.py", "WOFTChained"), ("WOFT_chained_multi_photo.py", "WOFTChainedMulti")):
        trk = _tracker(cfg)
        assert type(trk).__name__ == cls and trk._photo["iters"] == 10 and "photometric refinement of fitted frames (10 iterations" in \
            trk.solver_decision


# ---- 6. one batched call per frame -------------------------------------------------------------------------------------------------------
def test_one_batched_call_per_frame(monkeypatch, frames):
    monkeypatch.setenv("WOFT_FUSED", "1")
    trk = _tracker("WOFT_chained_multi.py", chain_photo_refine=6)
    trk.init(frames[0], U.stub_masks())
    trk.track(frames[1])                                             # (buffers allocated, library loaded)
    with pytest.MonkeyPatch.context() as patch:
        proxy = U.CountingLib(_lib.load())
        patch.setattr(_lib, "_lib", proxy)
        Hs, metas = trk.track(frames[2])
        torch.cuda.synchronize()
    calls = [c for c in proxy.calls if c.startswith("woft_photo")]
    assert calls == ["woft_photo_refine_multi"], calls
    assert [m.lost for m in metas] == [False, False, True]
