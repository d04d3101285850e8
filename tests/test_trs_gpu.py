"""The HIP RANSAC similarity estimator (csrc/trs.hip, homography.find_homography_TRS) on the GPU: the same per-hypothesis counts,
stop, best hypothesis, inlier mask and refit as the host restatement of cv2's loop (tests/trs_host.py), recovery of a known
similarity and the adaptive stop, the reference's API, a workspace no larger than it says, and the TRS tracker configs -- device
back end equal to the callable back end bit for bit, and a pose that stays on the ground truth among 40 % outliers."""
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import trs_host as th  # noqa: E402
from woft_amd import _lib, ops, synth  # noqa: E402
from woft_amd.homography import find_homography_TRS  # noqa: E402

W_IMG, H_IMG = 640, 480
_ANG = np.deg2rad(3.0)
S_TRUE = np.array([[1.05 * np.cos(_ANG), -1.05 * np.sin(_ANG), 12.0], [1.05 * np.sin(_ANG), 1.05 * np.cos(_ANG), -7.0],
                   [0.0, 0.0, 1.0]])
CORNERS = np.array([[0, 0], [W_IMG, 0], [W_IMG, H_IMG], [0, H_IMG]], np.float64)


def _proj(H, p):
    q = np.c_[p, np.ones(len(p))] @ np.asarray(H, np.float64).T
    return q[:, :2] / q[:, 2:]


def _corner_err(Ha, Hb):
    return float(np.linalg.norm(_proj(Ha, CORNERS) - _proj(Hb, CORNERS), axis=1).max())


def make_points(n, sigma, outliers, seed, H=S_TRUE):
    """Correspondences a -> S a (+ N(0, sigma) px); a fraction `outliers` of them moved 20 to 60 px away in a random direction.
    -> (pa, pb) float32 (n, 2), inlier ground truth (n,) bool."""
    rng = np.random.default_rng(seed)
    a = rng.random((n, 2)) * [W_IMG, H_IMG]
    b = _proj(H, a) + rng.normal(0.0, sigma, (n, 2)) * (sigma > 0)
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:int(round(outliers * n))]] = True
    ang = rng.random(out.sum()) * 2 * np.pi
    r = 20.0 + 40.0 * rng.random(out.sum())
    b[out] += np.c_[np.cos(ang), np.sin(ang)] * r[:, None]
    return a.astype(np.float32), b.astype(np.float32), ~out


def run_device(pa, pb, max_iters=10000, thr=3.0, conf=0.999, seed=0, refine=True, tail=0):
    """woft_trs on one set -> dict(H (3,3) float64, status, n_inliers, best_k, iterations, mask, counts, tail (the `tail` bytes
    behind the workspace, filled with 0xA5 before the call))."""
    n = pa.shape[0]
    a, b = torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda()
    Hout = torch.empty(9, device="cuda")
    st = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    info = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    mask = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    need = int(_lib.load().woft_trs_ws_bytes(n, max_iters))
    ws = torch.full((need + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    ops.trs(a, b, Hout, st, max_iters=max_iters, thr=thr, conf=conf, seed=seed, refine=refine, info=info, inlier_mask=mask, ws=ws)
    torch.cuda.synchronize()
    counts = ws[:4 * max_iters].view(torch.int32).cpu().numpy()          # (the workspace starts with the per-hypothesis counts)
    i = info.cpu().numpy()
    return dict(H=Hout.cpu().numpy().astype(np.float64).reshape(3, 3), status=int(st.item()), n_inliers=int(i[0]),
                best_k=int(i[1]), iterations=int(i[2]), mask=mask.cpu().numpy().astype(bool), counts=counts,
                tail=ws[need:].cpu().numpy())


def _expected_H(d, hyp, n, refine=True):
    """The host's fp64 model for the device's own decisions: the closed form over the device's mask where the refit runs, else
    the two-point model of the device's best hypothesis."""
    if refine and n > 2 and d["n_inliers"] > 2:
        m = th.refit(hyp.pa[d["mask"]], hyp.pb[d["mask"]])
        if m is not None:
            return th.to_H(m)
    return th.to_H(th.model2(hyp.pa, hyp.pb) if n == 2 else hyp.get(d["best_k"])[1])


# ---- 1. the same result as the host restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 500, 4097])                     # (4097: a one-point tail in a second scoring chunk)
@pytest.mark.parametrize("sigma", [0.0, 0.5])
@pytest.mark.parametrize("outliers", [0.0, 0.3, 0.6])
def test_same_result_as_the_host_restatement(n, sigma, outliers):
    max_iters = 1000
    for seed in (0, 1, 12345):
        pa, pb, _ = make_points(n, sigma, outliers, seed=100 * n + seed)
        d = run_device(pa, pb, max_iters=max_iters, seed=seed)
        h = th.trs_host(pa, pb, max_iters=max_iters, thr=3.0, conf=0.999, seed=seed)
        if n > 2:                           # (n == 2 is the direct model: nothing is sampled or scored)
            host_counts = np.array([h["hyp"].get(k)[2] for k in range(max_iters)])
            near = np.array([h["hyp"].get(k)[3] for k in range(max_iters)])
            diff = np.abs(d["counts"] - host_counts)
            assert np.all(diff <= near), (seed, np.flatnonzero(diff > near)[:10])
            if np.any(diff):
                continue                    # (a threshold tie decided differently: the selection may then differ legitimately)
        assert (d["status"], d["iterations"], d["best_k"], d["n_inliers"]) == \
            (h["status"], h["iterations"], h["best_k"], h["n_inliers"]), seed
        if h["status"] == 0:
            e64 = th.errors_f64(h["m"], pa, pb)
            tie = np.abs(e64 - 9.0) <= 1e-4 * 9.0
            assert np.array_equal(d["mask"] & ~tie, h["mask"] & ~tie), seed
            assert np.array_equal(d["H"][2], [0.0, 0.0, 1.0])
            err = _corner_err(d["H"], _expected_H(d, h["hyp"], n))
            assert err < 1e-3, (seed, err)
        else:
            assert np.isnan(d["H"]).all() and not d["mask"].any()


# ---- 2. recovery and stop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outliers,stop", [(0.0, 1), (0.3, 10), (0.6, 40)])
def test_recovery_and_stop(outliers, stop):
    for seed in (0, 1, 12345):
        pa, pb, gt = make_points(500, 0.0, outliers, 100 * 500 + seed)
        d = run_device(pa, pb, max_iters=1000, seed=seed)
        h = th.trs_host(pa, pb, max_iters=1000, thr=3.0, conf=0.999, seed=seed)
        assert d["status"] == 0 and d["iterations"] == h["iterations"] == stop, (seed, d["iterations"], h["iterations"])
        assert d["best_k"] == h["best_k"] and np.array_equal(d["mask"], gt) and d["n_inliers"] == int(gt.sum()), seed
        assert _corner_err(d["H"], S_TRUE) < 1e-3, (seed, _corner_err(d["H"], S_TRUE))
        pa, pb, gt = make_points(500, 0.5, outliers, 100 * 500 + seed)
        d = run_device(pa, pb, max_iters=1000, seed=seed)
        assert d["status"] == 0 and not np.any(d["mask"] & ~gt), seed
        assert _corner_err(d["H"], S_TRUE) < 0.5, (seed, _corner_err(d["H"], S_TRUE))


# ---- 3. API -----------------------------------------------------------------------------------------------------------------
def test_api():
    pa, pb, _ = make_points(300, 0.5, 0.3, 31)
    Hn = find_homography_TRS(pa[None], pb[None])
    assert isinstance(Hn, np.ndarray) and Hn.dtype == np.float64 and Hn.shape == (1, 3, 3)
    assert np.array_equal(Hn[0, 2], [0.0, 0.0, 1.0]) and Hn[0, 0, 0] == Hn[0, 1, 1] and Hn[0, 0, 1] == -Hn[0, 1, 0]
    assert _corner_err(Hn[0], S_TRUE) < 0.5
    Hc = find_homography_TRS(torch.from_numpy(pa[None]).cuda(), torch.from_numpy(pb[None]).cuda())
    assert Hc.is_cuda and Hc.dtype == torch.float64 and np.array_equal(Hc.cpu().numpy(), Hn)
    Hh = find_homography_TRS(torch.from_numpy(pa[None]), torch.from_numpy(pb[None]))
    assert Hh.device.type == "cpu" and Hh.dtype == torch.float64 and np.array_equal(Hh.numpy(), Hn)
    # weights are ignored; the same seed repeats bit for bit
    w = torch.rand(1, 300).cuda()
    Hw = find_homography_TRS(torch.from_numpy(pa[None]).cuda(), torch.from_numpy(pb[None]).cuda(), weights=w)
    assert np.array_equal(Hw.cpu().numpy(), Hn)
    assert np.array_equal(find_homography_TRS(pa[None], pb[None], seed=0), Hn)
    d0, d1 = run_device(pa, pb), run_device(pa, pb)
    assert np.array_equal(d0["H"], d1["H"]) and np.array_equal(d0["counts"], d1["counts"])
    # a batch: every element fitted independently with the same seed
    sets = [make_points(200 + 50 * i, 0.5, 0.2 * i, 40 + i)[:2] for i in range(3)]
    n = 200
    A = np.stack([s[0][:n] for s in sets])
    B = np.stack([s[1][:n] for s in sets])
    Hb = find_homography_TRS(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), seed=7)
    for i in range(3):
        Hi = find_homography_TRS(torch.from_numpy(A[i:i + 1]).cuda(), torch.from_numpy(B[i:i + 1]).cuda(), seed=7)
        assert np.array_equal(Hb[i].cpu().numpy(), Hi[0].cpu().numpy()), i
    # N = 1 raises before any launch; N = 2 is the exact solution
    with pytest.raises(AssertionError):
        find_homography_TRS(pa[None, :1], pb[None, :1])
    a2 = np.array([[10, 20], [300, 260]], np.float32)
    b2 = _proj(S_TRUE, a2).astype(np.float32)
    H2 = find_homography_TRS(a2[None], b2[None])[0]
    assert np.abs(_proj(H2, a2) - b2).max() < 1e-4
    d = run_device(a2, b2)
    assert (d["status"], d["n_inliers"], d["best_k"], d["iterations"]) == (0, 2, 0, 0) and d["mask"].all()
    # every A point identical: every model is degenerate -> H all NaN, status 2
    la = np.full((64, 2), 33.0, np.float32)
    lb = (la + np.arange(64, dtype=np.float32)[:, None]).astype(np.float32)
    d = run_device(la, lb, max_iters=200)
    assert d["status"] == 2 and np.isnan(d["H"]).all() and not d["mask"].any() and d["best_k"] == -1
    assert np.isnan(find_homography_TRS(la[None], lb[None], max_iters=200)).all()
    # refine=False: the two-point model of the best hypothesis, as stored in fp32
    pa, pb, _ = make_points(500, 0.5, 0.3, 32)
    d = run_device(pa, pb, max_iters=1000, seed=3, refine=False)
    hyp = th.Hypotheses(pa, pb, 3.0, 3)
    assert d["status"] == 0 and np.array_equal(d["H"], th.to_H(hyp.get(d["best_k"])[1]).astype(np.float32).astype(np.float64))
    assert not np.array_equal(d["H"], run_device(pa, pb, max_iters=1000, seed=3)["H"])


# ---- 4. scratch -------------------------------------------------------------------------------------------------------------
def test_scratch_untouched_beyond_its_size():
    pa, pb, gt = make_points(4097, 0.0, 0.3, 61)
    d = run_device(pa, pb, max_iters=1000, tail=256)
    assert d["status"] == 0 and np.array_equal(d["mask"], gt)
    assert d["tail"].size == 256 and np.all(d["tail"] == 0xA5)


# ---- 5. tracker -------------------------------------------------------------------------------------------------------------
def _load(name):
    from pytracking.utils.config import load_config
    if name == "reference_form":
        path = ROOT / "tests" / "configs" / "reference_forms_trs.py"
        m = types.ModuleType("tracker_config")
        m.__file__ = str(path)
        exec(compile(path.read_text(), str(path), "exec"), m.__dict__)
        return m.get_config()
    return load_config(ROOT / "pytracking" / "configs" / name)


def _tracker(name, sd, iters, device_solver=True):
    conf = _load(name)
    conf.flow_config.model = sd
    conf.flow_config.iters = iters
    if not device_solver:
        conf.device_solver = False
    trk = conf.tracker_class(conf)
    assert (trk._fused is not None) == device_solver, trk.solver_decision
    return trk


@pytest.mark.parametrize("name", ["WOFT_TRS.py", "reference_form"])
def test_tracker_device_back_end_equals_callable_back_end(name):
    H, W, iters, nframes = 136, 200, 3, 4
    sd = synth.make_state_dict(seed=7)
    template = synth.make_template(H, W, seq_id=8)
    frames = [synth.make_frame(template, t) for t in range(1, nframes + 1)]
    mask = synth.make_init_mask(H, W)
    runs = []
    for dev in (True, False):
        trk = _tracker(name, sd, iters, device_solver=dev)
        if dev:
            assert trk._fused["trs"] == dict(max_iters=10000, thr=3.0, conf=0.999) and "ransac" not in trk._fused
            assert trk.solver_decision.startswith("device back end")
        trk.init(template, mask)
        runs.append([trk.track(f) for f in frames])
    for (Ha, ma), (Hb, mb) in zip(*runs):
        assert ma.lost == mb.lost and ma.N_lost == mb.N_lost and bool(ma.global_H_success) == bool(mb.global_H_success)
        assert np.array_equal(Ha, Hb), np.abs(Ha - Hb).max()
        assert np.array_equal(ma.H_global_cur2init, mb.H_global_cur2init)


def seq_similarity(t, H, W):
    """S_t: template -> frame t of a similarity sequence (translation, rotation about the centre, zoom)."""
    cx, cy = W / 2.0, H / 2.0
    a, s = np.deg2rad(0.5 * t), 1.0 + 0.01 * t
    ca, sa = s * np.cos(a), s * np.sin(a)
    R = np.array([[ca, -sa, cx - ca * cx + sa * cy], [sa, ca, cy - sa * cx - ca * cy], [0, 0, 1.0]])
    T = np.array([[1, 0, 3.0 * t], [0, 1, -2.0 * t], [0, 0, 1.0]])
    return T @ R


def _inject_flow(trk, H, W, state, outliers, seed):
    """Replace the network's flow by the ground-truth correspondences of the similarity sequence, a fraction `outliers` of them
    moved by one common 25 px shift plus noise (a second, distracting motion)."""
    orig = trk.flower.compute_flow
    rng = np.random.default_rng(seed)

    def compute_flow(src, dst, **kw):
        src_xy, dst_xy, w = orig(src, dst, **kw)
        t = state["t"]
        St = seq_similarity(t, H, W)
        if src is trk.template_img:                          # global stage: template -> frame pre-warped by last_good_H2init
            M = trk.last_good_H2init @ St
        else:                                                # local stage: frame t-1 -> frame t
            M = St @ np.linalg.inv(seq_similarity(t - 1, H, W)) if t > 1 else St
        p = src_xy.double().cpu().numpy().T
        q = _proj(M, p)
        k = q.shape[0]
        out = rng.random(k) < outliers
        q[out] += np.array([25.0, 0.0]) + rng.normal(0, 2.0, (int(out.sum()), 2))
        dst_xy.copy_(torch.from_numpy(q.T.astype(np.float32)))
        return src_xy, dst_xy, w
    trk.flower.compute_flow = compute_flow


def _track_gt(name, outliers, sd, template, mask, H, W, nframes):
    trk = _tracker(name, sd, 2)
    trk.init(template, mask)
    state = {"t": 0}
    _inject_flow(trk, H, W, state, outliers, seed=1)
    errs = []
    for t in range(1, nframes + 1):
        state["t"] = t
        St = seq_similarity(t, H, W)
        frame = np.ascontiguousarray(np.clip(np.round(synth.warp_image_np(template, St)), 0, 255).astype(np.uint8))
        Hc, _ = trk.track(frame)
        c = np.array([[W / 4, H / 4], [3 * W / 4, H / 4], [3 * W / 4, 3 * H / 4], [W / 4, 3 * H / 4]])
        errs.append(float(np.abs(_proj(np.linalg.inv(Hc), c) - _proj(St, c)).max()))
    return errs


def test_tracker_pose_with_outliers_stays_on_the_ground_truth():
    H, W, nframes = 136, 200, 4
    sd = synth.make_state_dict(seed=7)
    template = synth.make_template(H, W, seq_id=8)
    mask = synth.make_init_mask(H, W)
    for name in ("WOFT_TRS.py", "reference_form"):
        for outliers in (0.0, 0.4):
            errs = _track_gt(name, outliers, sd, template, mask, H, W, nframes)
            assert max(errs) < 1.0, (name, outliers, errs)


def test_window_tracker_takes_the_estimator():
    """WOFTWindow inherits the solver: with the TRS preset the device back end equals the callable back end bit for bit."""
    from woft_amd import presets
    H, W, iters, nframes = 136, 200, 3, 3
    sd = synth.make_state_dict(seed=7)
    template = synth.make_template(H, W, seq_id=8)
    frames = [synth.make_frame(template, t) for t in range(1, nframes + 1)]
    mask = synth.make_init_mask(H, W)
    runs = []
    for dev in (True, False):
        conf = _load("WOFT_window.py")
        conf.H_estimator = presets.estimator_trs()
        conf.flow_config.model = sd
        conf.flow_config.iters = iters
        if not dev:
            conf.device_solver = False
        trk = conf.tracker_class(conf)
        assert type(trk).__name__ == "WOFTWindow" and (trk._fused is not None) == dev, trk.solver_decision
        if dev:
            assert trk._fused["trs"] == dict(max_iters=10000, thr=3.0, conf=0.999)
        trk.init(template, mask)
        runs.append([trk.track(f) for f in frames])
    for (Ha, ma), (Hb, mb) in zip(*runs):
        assert np.all(np.isfinite(Ha)) and ma.lost == mb.lost and np.array_equal(Ha, Hb), np.abs(Ha - Hb).max()
