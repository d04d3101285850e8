"""The visibility-weighted photometric refinement inside the chained trackers (config key `chain_photo_weights`; DESIGN.md section
30) on the stub provider of tests/chained_multi_util.py with the textured frames of tests/test_chained_photo_gpu.py: track()
returns what PhotoTemplate.refine makes of the fit's pose under the tracker's own map; the four trackers agree byte for byte where
they are stated to; a target with too little visible support keeps the fit's pose; one woft_photo_weights launch per frame whatever
K; and the keys' refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import chained_multi_util as U  # noqa: E402
import photo_weights_host as pw  # noqa: E402
from test_chained_photo_gpu import frames  # noqa: E402, F401  (the module's fixture: frame 0 and the frames rendered under U.motion)
from woft_amd import _lib, photo  # noqa: E402
from woft_amd.homography import compose_H  # noqa: E402

KEYS = dict(chain_photo_refine=6, chain_photo_weights="gate")
OCCLUDED = dict(raft_type="weighted_masked", occlude="left@3")       # visibility logit -6 on the left half of every flow into frame 3


def _config(name, raft_type="weighted", occlude=None, **keys):
    from pytracking.utils.config import load_config
    conf = load_config(U.ROOT / "pytracking" / "configs" / name)
    conf.flow_config.raft_type = raft_type
    conf.flow_config.of_class = lambda fc: U.AffineProvider(fc, occlude)
    conf.chain_deltas = U.S_DELTAS
    for k, v in keys.items():
        setattr(conf, k, v)
    return conf


def _tracker(name, **keys):
    conf = _config(name, **keys)
    return conf.tracker_class(conf)


def _plain(meta):
    """meta with its photo namespace as a tuple whose NaNs compare equal (a LOW_SUPPORT entry has no costs)."""
    out = type(meta)(**vars(meta))
    p = getattr(out, "photo", None)
    if p is not None:
        out.photo = tuple((k, "nan" if isinstance(v, float) and v != v else v) for k, v in sorted(vars(p).items()))
    return out


def _same(multi, singles, tag):
    U.assert_same_result([(Hs, [_plain(m) for m in metas]) for Hs, metas in multi],
                         [[(H, _plain(m)) for H, m in run] for run in singles], tag)


# ---- 1. the pose is the refinement under the tracker's map ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gate", "soft"])
@pytest.mark.parametrize("cfg", ["WOFT_chained.py", "WOFT_chained_window.py"])
def test_pose_is_the_refinement_under_the_trackers_map(frames, cfg, mode):
    mask = U.stub_masks()[0]
    keys = dict(chain_prewarp=False) if "window" in cfg else {}
    trk = _tracker(cfg, **OCCLUDED, **keys, chain_photo_refine=6, chain_photo_weights=mode, chain_photo_erode=1)
    assert f"refinement weighted by chain visibility ({mode}" in trk.solver_decision
    trk.init(frames[0], mask)
    pt = photo.PhotoTemplate(frames[0], mask)
    n_mask = np.count_nonzero(mask)
    for t in (1, 2, 3):
        H, meta = trk.track(frames[t])
        wmap = trk.photo_weight_map
        assert not meta.lost and isinstance(wmap, torch.Tensor) and wmap.is_cuda and tuple(wmap.shape) == (U.SH, U.SW)
        host_map = wmap.cpu().numpy()
        W, info = pt.refine(frames[t], np.linalg.inv(meta.H_flow_cur2init), iters=6, weights=wmap)
        assert info.best >= 0 and H.tobytes() == compose_H(np.linalg.inv(W)).tobytes()
        p = meta.photo
        assert (p.status, p.best, p.iterates) == (info.status, info.best, len(info.cost))
        assert p.support == np.count_nonzero((host_map > 0) & (mask > 0)) / n_mask
        near = host_map[11:37, 15:49]                            # the mask (rows 12 .. 35, columns 16 .. 47) and a pixel around it
        if t < 3:                                                # every chain valid and visible: nothing to erode
            assert np.all(near > 0) and p.support == 1.0
            assert np.all(near == 1) if mode == "gate" else (near.max() < 1 and near.min() > 0)
        else:                                                    # the left half is occluded; the erosion takes one more column
            assert np.all(near[:, :U.SW // 2 + 1 - 15] == 0) and np.all(near[:, U.SW // 2 + 1 - 15:] > 0)
            assert p.support == (48 - 33) / 32                   # (of the mask's columns 16 .. 47, 33 .. 47 are left)
            unweighted, _ = pt.refine(frames[t], np.linalg.inv(meta.H_flow_cur2init), iters=6)
            assert unweighted.tobytes() != W.tobytes()
        print(f"{cfg} {mode} frame {t}: support {p.support:.3f}, {p.status} after {p.iterates} iterates")


# ---- 2. the four trackers agree ------------------------------------------------------------------------------------------------------------
def _runs(frames, multi_cfg, single_cfg, masks, **keys):
    trk = _tracker(multi_cfg, **keys)
    trk.init(frames[0], masks)
    multi = [trk.track(f) for f in frames[1:5]]
    singles = []
    for m in masks:
        one = _tracker(single_cfg, **keys)
        one.init(frames[0], m)
        singles.append([one.track(f) for f in frames[1:5]])
    return trk, multi, singles


@pytest.mark.parametrize("route", ["batched", "loop"])
def test_multi_equals_single_trackers(monkeypatch, frames, route):
    monkeypatch.setenv("WOFT_FUSED", "0" if route == "loop" else "1")
    trk, multi, singles = _runs(frames, "WOFT_chained_multi.py", "WOFT_chained.py", U.stub_masks(), **OCCLUDED, **KEYS)
    assert trk._route == route and "refinement weighted by chain visibility" in trk.solver_decision
    _same(multi, singles, route)
    # frame 3: target 0 keeps 15 of its 32 columns and is refined, target 1 (columns 8 .. 35) keeps 3 of 28 and is not
    metas = multi[2][1]
    assert metas[0].photo.status != "LOW_SUPPORT" and metas[0].photo.support == 15 / 32
    assert (metas[1].photo.status, metas[1].photo.best, metas[1].photo.iterates) == ("LOW_SUPPORT", -1, 0)
    assert metas[1].photo.support == 3 / 28 and multi[2][0][1].tobytes() == metas[1].H_flow_cur2init.tobytes()
    assert metas[2].lost and not hasattr(metas[2], "photo")
    assert all(m.photo.support == 1.0 for f in (0, 1, 3) for m in multi[f][1][:2])


def test_window_tracker_on_whole_frames_equals_the_chained_tracker(frames):
    mask = U.stub_masks()[0]
    runs = []
    for cfg, extra in (("WOFT_chained.py", {}), ("WOFT_chained_window.py", dict(search_window_margin=None, chain_prewarp=False))):
        trk = _tracker(cfg, **OCCLUDED, **KEYS, **extra)
        trk.init(frames[0], mask)
        out = [trk.track(f) for f in frames[1:5]]
        for _, m in out:
            m.__dict__.pop("chain_window", None)                 # (the window tracker's own entry)
        runs.append(out)
    for (_, ma), (_, mb) in zip(*runs):                          # (the announcement: the window tracker's adds its own clause)
        if hasattr(ma, "solver_decision"):
            assert mb.solver_decision.startswith(ma.solver_decision) and "search windows" in mb.solver_decision
            del ma.solver_decision, mb.solver_decision
    _same([(H[None], [m]) for H, m in runs[1]], [runs[0]], "window")
    assert runs[0][2][1].photo.support == 15 / 32


def test_multi_window_with_one_mask_equals_the_window_tracker(monkeypatch, frames):
    monkeypatch.setenv("WOFT_FUSED", "1")
    trk, multi, singles = _runs(frames, "WOFT_chained_multi_window.py", "WOFT_chained_window.py", [U.stub_masks()[0]], **OCCLUDED,
                                **KEYS, chain_prewarp=False)
    assert trk._route == "batched"
    _same(multi, singles, "multi window")
    assert multi[2][1][0].photo.support == 15 / 32 and hasattr(multi[2][1][0], "chain_window")


# ---- 3. low support ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["WOFT_chained.py", "WOFT_chained_multi.py"])
def test_low_support_keeps_the_fits_pose(monkeypatch, frames, cfg):
    monkeypatch.setenv("WOFT_FUSED", "1")
    multi = "multi" in cfg
    trk = _tracker(cfg, **OCCLUDED, **KEYS, chain_photo_min_support=1.0)
    trk.init(frames[0], U.stub_masks()[:2] if multi else U.stub_masks()[0])
    for t in (1, 2, 3):
        H, meta = trk.track(frames[t])
        if multi:
            H, meta = H[0], meta[0]
        assert not meta.lost
        if t < 3:
            assert meta.photo.support == 1.0 and meta.photo.status != "LOW_SUPPORT" and meta.photo.best >= 0
    assert meta.photo.support < 1
    assert (meta.photo.status, meta.photo.best, meta.photo.iterates) == ("LOW_SUPPORT", -1, 0)
    assert H.tobytes() == meta.H_flow_cur2init.tobytes()
    state = trk._targets[0] if multi else trk
    assert state.prev_H2init.tobytes() == H.tobytes()


# ---- 4. one launch per frame, whatever K ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg, n_masks", [("WOFT_chained.py", 1), ("WOFT_chained_multi.py", 3), ("WOFT_chained_multi_window.py", 2)])
def test_one_weights_launch_per_frame(monkeypatch, frames, cfg, n_masks):
    monkeypatch.setenv("WOFT_FUSED", "1")
    keys = dict(chain_prewarp=False) if "window" in cfg else {}
    trk = _tracker(cfg, **OCCLUDED, **KEYS, **keys)
    trk.init(frames[0], U.stub_masks()[:n_masks] if n_masks > 1 else U.stub_masks()[0])
    trk.track(frames[1])                                             # (buffers allocated, library loaded)
    with pytest.MonkeyPatch.context() as patch:
        proxy = U.CountingLib(_lib.load())
        patch.setattr(_lib, "_lib", proxy)
        trk.track(frames[2])
        torch.cuda.synchronize()
    calls = [c for c in proxy.calls if c.startswith("woft_photo")]
    assert calls == ["woft_photo_weights", "woft_photo_refine" if n_masks == 1 else "woft_photo_refine_multi"], calls
    # the map was enqueued before the planar stage's first launch
    first_planar = min(i for i, c in enumerate(proxy.calls) if c.startswith("woft_chain_tc"))
    assert proxy.calls.index("woft_photo_weights") < first_planar
    assert trk.photo_weights_wait_s >= 0.0 and trk.host_wait_s >= trk.photo_weights_wait_s


# ---- 5. the keys ---------------------------------------------------------------------------------------------------------------------------
def test_the_key_needs_chain_photo_refine():
    for cfg in ("WOFT_chained.py", "WOFT_chained_multi.py", "WOFT_chained_window.py", "WOFT_chained_multi_window.py"):
        for extra in ({}, dict(chain_photo_refine=0), dict(chain_photo_refine=None)):
            with pytest.raises(ValueError, match="chain_photo_weights.*chain_photo_refine"):
                _tracker(cfg, chain_photo_weights="gate", **extra)


@pytest.mark.parametrize("keys", [dict(chain_photo_weights="hard"), dict(chain_photo_weights=True), dict(chain_photo_erode=5),
                                  dict(chain_photo_erode=-1), dict(chain_photo_erode=1.5), dict(chain_photo_erode=True),
                                  dict(chain_photo_min_support=1.5), dict(chain_photo_min_support=-0.1),
                                  dict(chain_photo_min_support=float("nan")), dict(chain_photo_min_support="half")])
def test_bad_values_raise(keys):
    for cfg in ("WOFT_chained_photo_occl.py", "WOFT_chained_multi_photo_occl.py"):
        with pytest.raises(ValueError, match="chain_photo_"):
            _tracker(cfg, **keys)


def test_the_occl_configs_and_the_key_absent(frames):
    for cfg, cls in (("WOFT_chained_photo_occl.py", "WOFTChained"), ("WOFT_chained_multi_photo_occl.py", "WOFTChainedMulti")):
        trk = _tracker(cfg)
        assert type(trk).__name__ == cls and trk._photo["iters"] == 10
        assert trk._photo_w == dict(mode="gate", erode=1, min_support=0.25)
        assert "refinement weighted by chain visibility (gate, vis >= 0.5, eroded by 1" in trk.solver_decision
    # a network that provides neither logit is allowed: the decision says what the map then does
    trk = _tracker("WOFT_chained_photo_occl.py", raft_type="orig")
    assert "only drops invalid chains" in trk.solver_decision
    trk.init(frames[0], U.stub_masks()[0])
    H, meta = trk.track(frames[1])
    assert not meta.lost and meta.photo.support == 1.0 and bool((trk.photo_weight_map[11:37, 15:49] == 1).all())
    # the key absent or None: no map, no launch, no support entry
    for extra in ({}, dict(chain_photo_weights=None)):
        trk = _tracker("WOFT_chained_photo.py", **extra)
        assert trk._photo_w is None and "weighted by chain visibility" not in trk.solver_decision
        trk.init(frames[0], U.stub_masks()[0])
        H, meta = trk.track(frames[1])
        assert trk.photo_weight_map is None and not hasattr(meta.photo, "support")
