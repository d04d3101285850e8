"""The HIP RANSAC estimator (csrc/ransac.hip, homography.find_homography_cvransac) on the GPU: the same per-hypothesis counts,
stop, best hypothesis and inlier mask as the host restatement of cv2's loop (tests/ransac_host.py), recovery of a known
homography, the adaptive stop, the reference's API, the full-frame case, and the RANSAC tracker configs -- device back end equal
to the callable back end bit for bit, and a pose that stays on the ground truth where the weighted least squares drifts."""
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import ransac_host as rh  # noqa: E402
from woft_amd import _lib, ops, synth  # noqa: E402
from woft_amd.homography import find_homography_cvransac  # noqa: E402

W_IMG, H_IMG = 640, 480
H_TRUE = np.array([[1.03, 0.04, 12.0], [-0.03, 0.97, -7.0], [1.2e-4, -8e-5, 1.0]])
CORNERS = np.array([[0, 0], [W_IMG, 0], [W_IMG, H_IMG], [0, H_IMG]], np.float64)


def _proj(H, p):
    q = np.c_[p, np.ones(len(p))] @ np.asarray(H, np.float64).T
    return q[:, :2] / q[:, 2:]


def _corner_err(Ha, Hb, rms=False):
    d = np.linalg.norm(_proj(Ha, CORNERS) - _proj(Hb, CORNERS), axis=1)
    return float(np.sqrt((d ** 2).mean())) if rms else float(d.max())


def make_points(n, sigma, outliers, seed, w=W_IMG, h=H_IMG, H=H_TRUE):
    """Correspondences a -> H a (+ N(0, sigma) px); a fraction `outliers` of them moved 20 to 60 px away in a random direction.
    -> (pa, pb) float32 (n, 2), inlier ground truth (n,) bool."""
    rng = np.random.default_rng(seed)
    a = rng.random((n, 2)) * [w, h]
    b = _proj(H, a) + rng.normal(0.0, sigma, (n, 2)) * (sigma > 0)
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:int(round(outliers * n))]] = True
    ang = rng.random(out.sum()) * 2 * np.pi
    r = 20.0 + 40.0 * rng.random(out.sum())
    b[out] += np.c_[np.cos(ang), np.sin(ang)] * r[:, None]
    return a.astype(np.float32), b.astype(np.float32), ~out


def run_device(pa, pb, max_iters=10000, thr=3.0, conf=0.995, seed=0, refine=True):
    """woft_ransac on one set -> dict(H (3,3) float64, status, n_inliers, best_k, iterations, mask, counts)."""
    n = pa.shape[0]
    a, b = torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda()
    Hout = torch.empty(9, device="cuda")
    st = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    info = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    mask = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    ws = torch.empty(int(_lib.load().woft_ransac_ws_bytes(n, max_iters)), dtype=torch.uint8, device="cuda")
    ops.ransac(a, b, Hout, st, max_iters=max_iters, thr=thr, conf=conf, seed=seed, refine=refine, info=info, inlier_mask=mask,
               ws=ws)
    torch.cuda.synchronize()
    counts = ws[:4 * max_iters].view(torch.int32).cpu().numpy()          # (the workspace starts with the per-hypothesis counts)
    i = info.cpu().numpy()
    return dict(H=Hout.cpu().numpy().astype(np.float64).reshape(3, 3), status=int(st.item()), n_inliers=int(i[0]),
                best_k=int(i[1]), iterations=int(i[2]), mask=mask.cpu().numpy().astype(bool), counts=counts)


# ---- 1. the same result as the host restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 500, 4096])
@pytest.mark.parametrize("sigma", [0.0, 0.5])
@pytest.mark.parametrize("outliers", [0.0, 0.3, 0.6])
def test_same_result_as_the_host_restatement(n, sigma, outliers):
    max_iters = 1000
    for seed in (0, 1, 12345):
        pa, pb, _ = make_points(n, sigma, outliers, seed=100 * n + seed)
        d = run_device(pa, pb, max_iters=max_iters, seed=seed)
        h = rh.ransac_host(pa, pb, max_iters=max_iters, thr=3.0, conf=0.995, seed=seed)
        host_counts = np.array([h["hyp"].get(k)[2] for k in range(max_iters)])
        near = np.array([h["hyp"].get(k)[3] for k in range(max_iters)])
        diff = np.abs(d["counts"] - host_counts)
        assert np.all(diff <= near), (seed, np.flatnonzero(diff > near)[:10])
        if np.any(diff):
            continue                        # (a threshold tie decided differently: the selection may then differ legitimately)
        assert (d["status"], d["iterations"], d["best_k"], d["n_inliers"]) == \
            (h["status"], h["iterations"], h["best_k"], h["n_inliers"]), seed
        if h["status"] == 0:
            Hb = np.array(h["H"]).reshape(3, 3)
            e64 = rh.errors_f64(Hb.reshape(-1), pa, pb)
            tie = np.abs(e64 - 9.0) <= 1e-4 * 9.0
            assert np.array_equal(d["mask"] & ~tie, h["mask"] & ~tie), seed
        else:
            assert np.isnan(d["H"]).all() and not d["mask"].any()


# ---- 2. recovery ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outliers", [0.0, 0.3, 0.6])
def test_recovery_and_refinement(outliers):
    for seed in (3, 4):
        pa, pb, gt = make_points(500, 0.0, outliers, seed)
        d = run_device(pa, pb, seed=seed)
        assert d["status"] == 0 and np.array_equal(d["mask"], gt)
        assert _corner_err(d["H"], H_TRUE) < 1e-3, _corner_err(d["H"], H_TRUE)
        pa, pb, gt = make_points(500, 0.5, outliers, seed)
        d = run_device(pa, pb, seed=seed)
        m = d["mask"]                       # (inliers of the best 4-point model: noisy inliers near 3 px may fall out of it)
        assert d["status"] == 0 and not np.any(m & ~gt) and m.sum() >= 0.9 * gt.sum()
        opt = rh.geometric_optimum(d["H"], pa[m], pb[m])
        assert _corner_err(d["H"], opt, rms=True) < 1e-3, _corner_err(d["H"], opt, rms=True)
        # the LM start: woft_hfit's DLT over the same inliers; LM never raises the inlier error above it
        a, b = torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda()
        Hd, sd = torch.empty(9, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.hfit(a, b, torch.from_numpy(m.astype(np.float32)).cuda(), Hd, sd)
        Hd = Hd.cpu().numpy().astype(np.float64)
        e_dlt = rh.errors_f64(Hd / Hd[8], pa[m], pb[m]).sum()
        e_lm = rh.errors_f64(d["H"].reshape(-1), pa[m], pb[m]).sum()
        assert int(sd.item()) == 0 and e_lm <= e_dlt * (1 + 1e-6), (e_lm, e_dlt)


# ---- 3. adaptive stop -------------------------------------------------------------------------------------------------------
def test_adaptive_stop():
    pa, pb, _ = make_points(500, 0.0, 0.0, 21)
    d = run_device(pa, pb)
    assert d["iterations"] == 1 and d["best_k"] == 0 and d["n_inliers"] == 500     # (every point an inlier: niters -> 0)
    for seed in (0, 5):
        pa, pb, _ = make_points(500, 0.0, 0.6, 22 + seed)
        d = run_device(pa, pb, seed=seed)
        h = rh.ransac_host(pa, pb, max_iters=10000, thr=3.0, conf=0.995, seed=seed)
        assert d["iterations"] == h["iterations"] and d["best_k"] == h["best_k"], (d["iterations"], h["iterations"])
        assert 150 <= d["iterations"] <= 260, d["iterations"]          # (~204 for 40 % inliers at confidence 0.995)


# ---- 4. API -----------------------------------------------------------------------------------------------------------------
def test_api():
    pa, pb, _ = make_points(300, 0.5, 0.3, 31)
    Hn = find_homography_cvransac(pa[None], pb[None], max_iters=10000, thr=3)
    assert isinstance(Hn, np.ndarray) and Hn.dtype == np.float64 and Hn.shape == (1, 3, 3) and Hn[0, 2, 2] == 1.0
    Hc = find_homography_cvransac(torch.from_numpy(pa[None]).cuda(), torch.from_numpy(pb[None]).cuda(), max_iters=10000, thr=3)
    assert Hc.is_cuda and Hc.dtype == torch.float64 and np.array_equal(Hc.cpu().numpy(), Hn)
    Hh = find_homography_cvransac(torch.from_numpy(pa[None]), torch.from_numpy(pb[None]), max_iters=10000, thr=3)
    assert Hh.device.type == "cpu" and Hh.dtype == torch.float64 and np.array_equal(Hh.numpy(), Hn)
    # weights are ignored; the same seed repeats bit for bit
    w = torch.rand(1, 300).cuda()
    Hw = find_homography_cvransac(torch.from_numpy(pa[None]).cuda(), torch.from_numpy(pb[None]).cuda(), weights=w, thr=3)
    assert np.array_equal(Hw.cpu().numpy(), Hn)
    assert np.array_equal(find_homography_cvransac(pa[None], pb[None], thr=3), Hn)
    # a batch: every element fitted independently with the same seed
    sets = [make_points(200 + 50 * i, 0.5, 0.2 * i, 40 + i)[:2] for i in range(3)]
    n = 200
    A = np.stack([s[0][:n] for s in sets])
    B = np.stack([s[1][:n] for s in sets])
    Hb = find_homography_cvransac(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), thr=3, seed=7)
    for i in range(3):
        Hi = find_homography_cvransac(torch.from_numpy(A[i:i + 1]).cuda(), torch.from_numpy(B[i:i + 1]).cuda(), thr=3, seed=7)
        assert np.array_equal(Hb[i].cpu().numpy(), Hi[0].cpu().numpy()), i
    # N = 3 raises before any launch; N = 4 is the exact solution
    with pytest.raises(AssertionError):
        find_homography_cvransac(pa[None, :3], pb[None, :3])
    a4 = np.array([[10, 10], [300, 20], [320, 260], [15, 240]], np.float32)
    b4 = _proj(H_TRUE, a4).astype(np.float32)
    H4 = find_homography_cvransac(a4[None], b4[None])[0]
    assert np.abs(_proj(H4, a4) - b4).max() < 1e-3
    d = run_device(a4, b4)
    assert (d["status"], d["n_inliers"], d["best_k"], d["iterations"]) == (0, 4, 0, 0) and d["mask"].all()
    # all points exactly on one line (integer coordinates: exact in fp32): no sample passes the check -> H all NaN, status 2
    i = np.arange(64, dtype=np.float32)
    la = np.stack([10 + 6 * i, 20 + 3 * i], 1).astype(np.float32)
    lb = (la + 3).astype(np.float32)
    d = run_device(la, lb)
    assert d["status"] == 2 and np.isnan(d["H"]).all() and not d["mask"].any() and d["best_k"] == -1
    assert np.isnan(find_homography_cvransac(la[None], lb[None])).all()


# ---- 5. large N -------------------------------------------------------------------------------------------------------------
def test_full_frame_correspondences():
    n = 1920 * 1080
    pa, pb, gt = make_points(n, 0.0, 0.4, 51, w=1920, h=1080)
    d = run_device(pa, pb, max_iters=200)
    assert d["status"] == 0 and np.array_equal(d["mask"], gt) and d["n_inliers"] == int(gt.sum())
    a, b = torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda()
    Hout, st = torch.empty(9, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = ops.ransac_ws(n, 200)
    ops.ransac(a, b, Hout, st, max_iters=200, thr=3.0, ws=ws)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.ransac(a, b, Hout, st, max_iters=200, thr=3.0, ws=ws)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    print(f"\nRANSAC fit, N = {n}, 200 hypotheses, 40 % outliers: {ms:.2f} ms (one call, synchronised)")
    assert _corner_err(Hout.cpu().numpy().astype(np.float64).reshape(3, 3), H_TRUE) < 1e-2


# ---- 6. tracker -------------------------------------------------------------------------------------------------------------
def _load(name):
    from pytracking.utils.config import load_config
    if name == "reference_form":
        import types
        path = ROOT / "tests" / "configs" / "reference_forms_ransac.py"
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


@pytest.mark.parametrize("name", ["WOFT_RANSAC.py", "reference_form"])
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
            assert trk._fused["ransac"] == dict(max_iters=10000, thr=3.0, conf=0.995)
        trk.init(template, mask)
        runs.append([trk.track(f) for f in frames])
    for (Ha, ma), (Hb, mb) in zip(*runs):
        assert ma.lost == mb.lost and ma.N_lost == mb.N_lost and bool(ma.global_H_success) == bool(mb.global_H_success)
        assert np.array_equal(Ha, Hb), np.abs(Ha - Hb).max()
        assert np.array_equal(ma.H_global_cur2init, mb.H_global_cur2init)


def _inject_flow(trk, H, W, state, outliers, seed):
    """Replace the network's flow by the ground-truth correspondences of the synthetic sequence, a fraction `outliers` of them
    moved by one common 25 px shift plus noise (a second, distracting motion)."""
    orig = trk.flower.compute_flow
    rng = np.random.default_rng(seed)

    def compute_flow(src, dst, **kw):
        src_xy, dst_xy, w = orig(src, dst, **kw)
        t = state["t"]
        Ht = synth.seq_homography(t, H, W)
        if src is trk.template_img:                          # global stage: template -> frame pre-warped by last_good_H2init
            M = trk.last_good_H2init @ Ht
        else:                                                # local stage: frame t-1 -> frame t
            M = Ht @ np.linalg.inv(synth.seq_homography(t - 1, H, W)) if t > 1 else Ht
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
        Hc, _ = trk.track(synth.make_frame(template, t))
        Ht = synth.seq_homography(t, H, W)
        c = np.array([[W / 4, H / 4], [3 * W / 4, H / 4], [3 * W / 4, 3 * H / 4], [W / 4, 3 * H / 4]])
        errs.append(float(np.abs(_proj(np.linalg.inv(Hc), c) - _proj(Ht, c)).max()))
    return errs


def test_tracker_pose_with_outliers_ransac_holds_where_weighted_lsq_drifts():
    H, W, nframes = 136, 200, 4
    sd = synth.make_state_dict(seed=7)
    template = synth.make_template(H, W, seq_id=8)
    mask = synth.make_init_mask(H, W)
    for name in ("WOFT_RANSAC.py", "reference_form"):
        errs = _track_gt(name, 0.0, sd, template, mask, H, W, nframes)
        assert max(errs) < 1.0, (name, errs)
        errs = _track_gt(name, 0.4, sd, template, mask, H, W, nframes)
        assert max(errs) < 1.0, (name, errs)
    lsq = _track_gt("WOFT.py", 0.4, sd, template, mask, H, W, nframes)
    assert max(lsq) > 3.0, lsq
