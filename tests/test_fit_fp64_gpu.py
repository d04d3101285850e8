"""The homography fit kernels (csrc/hfit.hip: the one-workgroup `hfit_kernel`, the streaming pipeline, `woft_hfit_step`) and
the inlier test (`woft_inlier_frac`) against float64 restatements (tests/fp64_refs.py), tightly enough to see ONE
correspondence dropped or counted twice.

Sentinel method: a correspondence displaced by 40 px with a weight large enough to move the fp64 corners by >= 1 px is placed
in turn at the indices where the MFMA pair loop, the grid-stride loops and the workgroup partials change hands (0, 1, 31, 32,
255, 256, 2047, 2048, n-2, n-1).  Every case first checks that the fp64 fit with the sentinel differs from the fp64 fit with
that correspondence undisplaced by >= 20x the tolerance (so a kernel that lost or doubled it would fail), then that the kernel
agrees with the fp64 fit within the tolerance.  Errors are corner errors at the bounding box of the points, in pixels.

Tolerance: the kernel builds the rows in fp32 and rounds the normalised solution and H to fp32; a CPU emulation of exactly that
arithmetic lands within 3e-4 px of the fp64 fit on every shape used here (4K-range and 1700 x 920 boxes), and 6e-4 px on a
4-px box with a 4-px sentinel (conditioning of the projective terms).  TOL is 1e-3 px and TOL_BOX 5e-3 px.  Run with -s to see the
measured worst error and the smallest self-check margin of each family."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_refs as R  # noqa: E402

TOL = 1e-3
TOL_BOX = 5e-3
TOL_IRLS = 5e-3
MARGIN = 20.0
SENTINEL_IDX = (0, 1, 31, 32, 255, 256, 2047, 2048)
_STATS = {}


def _note(family, err, margin):
    e, m = _STATS.get(family, (0.0, math.inf))
    _STATS[family] = (max(e, err), min(m, margin))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam, (e, m) in sorted(_STATS.items()):
        print(f"\n[fit fp64] {fam}: worst kernel error {e:.3e} px, smallest self-check shift / tolerance {m:.1f}")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from woft_amd import _lib
    return _lib


def _synthetic(n, seed, lo=(100, 80), hi=(1800, 1000), outliers=0.1):
    """As test_homography_gpu._synthetic, in a box of choice: numpy float32 a, b (n, 2), w (n,)."""
    rs = np.random.RandomState(seed)
    Hgt = np.array([[1.02, 0.03, 12.0], [-0.02, 0.98, -7.0], [2e-5, -1e-5, 1.0]])
    a = np.stack([rs.uniform(lo[0], hi[0], n), rs.uniform(lo[1], hi[1], n)], 1)
    ah = np.concatenate([a, np.ones((n, 1))], 1) @ Hgt.T
    b = ah[:, :2] / ah[:, 2:] + rs.normal(0, 0.3, (n, 2))
    no = int(outliers * n)
    b[:no] += rs.uniform(-80, 80, (no, 2))
    w = rs.uniform(0.05, 1.0, n)
    w[:no] *= 0.2
    return a.astype(np.float32), b.astype(np.float32), w.astype(np.float32)


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _fit(lib, pa, pb, w, path, n_max=None, count=None, reweight=0, huber_k=1.0, n_irls=0):
    """One fit on the device -> (H (3, 3) float32 numpy, status).  path: 'ops' (ops.hfit, n <= 2048: the one-workgroup
    kernel), 'single' (raw ABI, ws = NULL: the one-workgroup kernel at any n), 'stream' (raw ABI with the workspace)."""
    from woft_amd import ops
    a, b, ww = (_dev(x) if not isinstance(x, torch.Tensor) else x for x in (pa, pb, w))
    n = a.shape[0] if n_max is None else n_max
    Hd = torch.full((9,), 777.0, device="cuda")
    st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    if path == "ops":
        assert n <= ops.HFIT_SINGLE_MAX and n_max is None
        ops.hfit(a, b, ww, Hd, st, count=cnt, reweight=reweight, huber_k=huber_k, n_irls=n_irls)
    else:
        ws = ops.hfit_ws() if path == "stream" else None
        lib.check(lib.load().woft_hfit(a.data_ptr(), b.data_ptr(), lib.ptr(ww), n, lib.ptr(cnt), reweight, float(huber_k),
                                       n_irls, lib.ptr(ws), Hd.data_ptr(), st.data_ptr(), lib.stream_ptr()), "woft_hfit")
    torch.cuda.synchronize()
    return Hd.cpu().numpy().reshape(3, 3), int(st.item())


def _sentinel(a, b, w, idx, corners, need, disp=40.0):
    """b, w with correspondence idx displaced by `disp` (40) px and its weight raised until the fp64 corners move by >= need px
    (w None: unweighted, the displacement alone).  -> (b_s, w_s, fp64 fit with, fp64 fit without, shift)."""
    b_s = b.copy()
    b_s[idx] += np.float32([disp, -0.75 * disp])
    H0 = R.fit(a, b, w)
    if w is None:
        H1 = R.fit(a, b_s, None)
        return b_s, None, H1, H0, R.corner_err(H1, H0, corners)
    w_s = w.copy()
    wv = 1.0
    while True:
        w_s[idx] = np.float32(wv)
        H1 = R.fit(a, b_s, w_s)
        shift = R.corner_err(H1, H0, corners)
        if shift >= need or wv >= 4096:
            return b_s, w_s, H1, H0, shift
        wv *= 2


def _positions(n):
    return sorted({i for i in SENTINEL_IDX + (n - 2, n - 1) if 0 <= i < n})


def _sentinel_case(lib, family, a, b, w, idx, path, tol, corners=None, disp=40.0, need=1.0, **kw):
    corners = R.box_corners(a) if corners is None else corners
    b_s, w_s, H1, H0, shift = _sentinel(a, b, w, idx, corners, max(need, MARGIN * tol), disp)
    assert shift >= MARGIN * tol, f"self-check: the sentinel at {idx} moves the fp64 fit by {shift:.3e} px only"
    H, st = _fit(lib, a, b_s, w_s, path, **kw)
    assert st == 0
    err = R.corner_err(H, H1, corners)
    _note(family, err, shift / tol)
    assert err <= tol, f"{family}: sentinel at {idx}: kernel {err:.3e} px from the fp64 fit (tol {tol:.0e})"
    return H


@pytest.mark.parametrize("n", [4, 5, 6, 7, 31, 32, 33, 63, 64, 65, 500, 1023, 1024, 1025, 2047, 2048])
def test_sentinel_sweep_single_workgroup(lib, n):
    a, b, w = _synthetic(n, seed=n, outliers=0.1 if n >= 10 else 0.0)
    for idx in _positions(n):
        _sentinel_case(lib, "single kernel (ops.hfit)", a, b, w, idx, "ops", TOL)


@pytest.mark.parametrize("n,path", [(2049, "single"), (4097, "single"), (8192, "single"),
                                    (2049, "stream"), (8193, "stream"), (20000, "stream")])
def test_sentinel_sweep_large(lib, n, path):
    a, b, w = _synthetic(n, seed=n + 1)
    for idx in _positions(n):
        _sentinel_case(lib, f"{path} kernel, n > 2048", a, b, w, idx, path, TOL)


@pytest.mark.parametrize("path,n", [("ops", 500), ("stream", 3000)])
def test_weights_and_geometry(lib, path, n):
    """Weights None / random / exact zeros on rows with wild coordinates, points in a 4-px box, 4K-range coordinates --
    each with the sentinel at both ends and in the middle of the first pair block."""
    a, b, w = _synthetic(n, seed=11)
    for idx in (0, 33, n - 1):
        # unweighted: the sentinel's displacement alone (n small enough for one point to matter)
        if path == "ops":
            _sentinel_case(lib, "weights None", a, b, None, idx, path, TOL)
        _sentinel_case(lib, "weights random", a, b, w, idx, path, TOL)
        # zero weights on rows whose coordinates are far outside the frame: they only move the normalisation
        aw, bw, ww = a.copy(), b.copy(), w.copy()
        wild = np.arange(5, n, 97)
        aw[wild] = np.float32([2.0e4, -1.5e4])
        bw[wild] = np.float32([-3.0e4, 2.5e4])
        ww[wild] = 0.0
        _sentinel_case(lib, "zero weights on wild rows", aw, bw, ww, idx, path, TOL, corners=R.box_corners(a))
    for idx in (1, n - 2):
        # (in a 4-px box: no 80-px outliers and a 4-px sentinel, or the fp64 fit itself is no homography one would track)
        a4, b4, w4 = _synthetic(n, seed=12, lo=(500, 300), hi=(504, 304), outliers=0.0)
        _sentinel_case(lib, "4-px box", a4, b4, w4, idx, path, TOL_BOX, disp=4.0, need=0.2)
        ak, bk, wk = _synthetic(n, seed=13, lo=(0, 0), hi=(3840, 2160))
        _sentinel_case(lib, "4K range", ak, bk, wk, idx, path, TOL)


def test_device_count_with_poisoned_tail(lib):
    """count < n_max, NaN in pa, pb and w beyond count: the one-workgroup kernel is bit-identical to n_max = count; the
    streaming pipeline (its partitioning follows n_max) agrees with n_max = count within 1e-6 px; both meet the fp64 fit."""
    for n_max, count, path in ((1024, 700, "ops"), (2048, 33, "ops"), (8192, 5000, "stream"), (8192, 1500, "stream"),
                               (4097, 2049, "single")):
        a, b, w = _synthetic(n_max, seed=n_max + count)
        for arr in (a, b):
            arr[count:] = np.nan
        w[count:] = np.nan
        Hc, st = _fit(lib, a, b, w, path if path != "ops" else "single", n_max=n_max, count=count)
        assert st == 0 and np.isfinite(Hc).all()
        corners = R.box_corners(a[:count])
        Href = R.fit(a[:count], b[:count], w[:count])
        err = R.corner_err(Hc, Href, corners)
        _note("device count", err, math.inf)
        assert err <= TOL, (n_max, count, err)
        sub = (a[:count].copy(), b[:count].copy(), w[:count].copy())
        if path in ("ops", "single") or count > 2048:
            Hn, st = _fit(lib, *sub, "stream" if path == "stream" else "single")
            assert st == 0
            if path == "stream":
                assert R.corner_err(Hc, Hn, corners) <= 1e-6, (n_max, count)
            else:
                assert np.array_equal(Hc, Hn), (n_max, count)
        else:                                # count <= 2048 < n_max: the same points through the one-workgroup kernel
            Hn, st = _fit(lib, *sub, "single")
            assert st == 0 and R.corner_err(Hc, Hn, corners) <= TOL


def test_singular_system_gives_status_2_and_nan(lib):
    """All correspondences identical: the normalised points are exactly 0 (power-of-two coordinates keep s * a + t exact),
    the Gram matrix has a zero pivot, status 2 and an all-NaN H on both paths, with and without IRLS."""
    for n, path in ((600, "ops"), (3000, "single"), (3000, "stream")):
        a = np.tile(np.float32([[512.0, 256.0]]), (n, 1))
        b = np.tile(np.float32([[1024.0, 128.0]]), (n, 1))
        for kw in (dict(), dict(reweight=2, huber_k=1.0, n_irls=3)):
            H, st = _fit(lib, a, b, np.ones(n, np.float32), path, **kw)
            assert st == 2 and np.isnan(H).all(), (n, path, kw, st)


@pytest.mark.parametrize("n", [1500, 3000])
def test_irls_huber_that_bites(lib, n):
    """Huber with k = 1 (continuous at |r| = k) on weights scaled to 20..100, so that the outliers' algebraic residuals exceed
    k: n_irls = 1..5 against the fp64 IRLS oracle; the single-workgroup and streaming kernels agree with each other."""
    a, b, w = _synthetic(n, seed=n + 5, outliers=0.2)
    w = (20.0 + 80.0 * (w - w.min()) / (w.max() - w.min())).astype(np.float32)
    corners = R.box_corners(a)
    H_plain = R.fit(a, b, w)
    for n_irls in range(1, 6):
        Href = R.fit_irls(a, b, w, huber_k=1.0, n_iter=n_irls)
        shift = R.corner_err(Href, H_plain, corners)
        assert shift >= MARGIN * TOL_IRLS, f"self-check: Huber(1) moves the fp64 fit by {shift:.3e} px only"
        out = {}
        for path in ("single", "stream") if n > 2048 else ("ops",):
            H, st = _fit(lib, a, b, w, path, reweight=2, huber_k=1.0, n_irls=n_irls)
            assert st == 0
            err = R.corner_err(H, Href, corners)
            _note("IRLS Huber(1)", err, shift / TOL_IRLS)
            assert err <= TOL_IRLS, (n_irls, path, err)
            out[path] = H
        if len(out) == 2:
            assert R.corner_err(out["single"], out["stream"], corners) <= TOL, n_irls


def _ws_sol_norm(ws):
    """The streaming workspace's sol[8] and norm[6] floats (csrc/hfit.hip mws_layout: after the G x (4 + 2 + 81) doubles)."""
    off = 1024 * (4 + 2 + 81) * 8
    f = ws[off:off + 64].clone().view(torch.float32).cpu().numpy()
    return f[:8].astype(np.float64), f[8:14].astype(np.float64)


def test_hfit_step_residuals_and_singular_after_good_fit(lib):
    """woft_hfit_step: the residuals are the fp64 A x - b of the step's own solution (within the fp32 rounding of a
    9-term dot product), slots past 2n stay untouched.  Then a singular fit on the same scratch: status 2, NaN H and NaN
    residuals -- not the residuals of the previous fit's solution left in the scratch."""
    from woft_amd import ops
    n = 3000
    a, b, w = _synthetic(n, seed=21)
    pa, pb, pw = _dev(a), _dev(b), _dev(w)
    ws = ops.hfit_ws()
    res = torch.full((2 * n + 64,), 12345.0, device="cuda")
    Hd, st = torch.zeros(9, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.hfit_step(pa, pb, pw, None, True, res, Hd, st, ws=ws)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    sol, norm = _ws_sol_norm(ws)
    r = res.cpu().numpy()
    assert np.all(r[2 * n:] == 12345.0)
    ref, mag = R.residuals(a, b, w, sol, norm)
    bound = 32 * R.U32 * mag
    err = np.abs(r[:2 * n] - ref)
    assert np.all(err <= bound), f"residuals: worst {float(err.max()):.3e}, worst ratio {float((err / bound).max()):.2f}"
    assert R.corner_err(Hd.cpu().numpy().reshape(3, 3), R.fit(a, b, w), R.box_corners(a)) <= TOL
    # a re-weighted step: the solution changes, the residuals follow it
    rew = torch.from_numpy(np.sqrt(1.0 / (np.abs(ref) + 1e-8)).astype(np.float32)).cuda()
    ops.hfit_step(pa, pb, pw, rew, False, res, Hd, st, ws=ws)
    torch.cuda.synchronize()
    sol2, norm2 = _ws_sol_norm(ws)
    assert int(st.item()) == 0 and not np.array_equal(sol2, sol) and np.array_equal(norm2, norm)
    ref2, mag2 = R.residuals(a, b, w, sol2, norm2)
    assert np.all(np.abs(res.cpu().numpy()[:2 * n] - ref2) <= 32 * R.U32 * mag2)
    # singular fit on the same scratch
    same = torch.from_numpy(np.tile(np.float32([[512.0, 256.0]]), (n, 1))).cuda()
    same_b = torch.from_numpy(np.tile(np.float32([[1024.0, 128.0]]), (n, 1))).cuda()
    res.fill_(12345.0)
    ops.hfit_step(same, same_b, pw, None, True, res, Hd, st, ws=ws)
    torch.cuda.synchronize()
    assert int(st.item()) == 2 and bool(torch.isnan(Hd).all())
    r = res.cpu().numpy()
    assert np.isnan(r[:2 * n]).all(), "residuals of a singular step must be NaN (stale solution in the scratch)"
    assert np.all(r[2 * n:] == 12345.0)


def _inlier_points(n, seed, thr):
    """Points whose fp64 distance to their partner spreads over [0, 2 thr], and a homography with a horizon line at
    x = -1000 + 25 y / 1000 ... (h6 = 1e-3, h7 = -2.5e-5)."""
    rs = np.random.RandomState(seed)
    H = np.array([[0.98, 0.02, 15.0], [-0.01, 1.01, -4.0], [1e-3, -2.5e-5, 1.0]], np.float32)
    a = np.stack([rs.uniform(0, 1900, n), rs.uniform(0, 1000, n)], 1)
    ah = np.concatenate([a, np.ones((n, 1))], 1) @ H.astype(np.float64).T
    proj = ah[:, :2] / ah[:, 2:]
    ang = rs.uniform(0, 2 * np.pi, n)
    rad = rs.uniform(0, 2 * thr, n)
    b = proj + np.stack([np.cos(ang), np.sin(ang)], 1) * rad[:, None]
    return H, a.astype(np.float32), b.astype(np.float32)


def _frac(lib, a, b, H, thr, n_max=None, count=None):
    from woft_amd import ops
    pa, pb = _dev(a), _dev(b)
    fr = torch.full((1,), -1.0, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    if n_max is None:
        ops.inlier_frac(pa, pb, _dev(H.reshape(9)), fr, thr=thr, count=cnt)
    else:
        Hd = _dev(H.reshape(9))
        lib.check(lib.load().woft_inlier_frac(pa.data_ptr(), pb.data_ptr(), n_max, lib.ptr(cnt), Hd.data_ptr(), float(thr),
                                              fr.data_ptr(), lib.stream_ptr()), "woft_inlier_frac")
    torch.cuda.synchronize()
    return float(fr.item())


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 5000])
def test_inlier_frac_count_is_exact(lib, n):
    thr = 5.0
    H, a, b = _inlier_points(n, seed=n, thr=thr)
    fr = _frac(lib, a, b, H, thr)
    k = int(round(fr * n))
    assert abs(k - fr * n) < 1e-3
    count, lo, hi = R.inlier_count(H, a, b, thr)
    assert lo <= k <= hi, (n, k, count, lo, hi)
    _note("inlier count: points either side of thr (a count, not px)", float(hi - lo), math.inf)


def test_inlier_frac_device_count_and_horizon(lib):
    thr = 5.0
    n_max, count = 2000, 1500
    H, a, b = _inlier_points(n_max, seed=31, thr=thr)
    # 300 points near the horizon line pz = 0, both sides: |pz| in [0.05, 0.5] with the partner at the fp64 projection
    # (inliers thousands of px away) or 50 px off it, and |pz| in [1e-4, 1e-2] with the partner at the point itself
    rs = np.random.RandomState(32)
    hz = np.arange(100, 400)
    y = rs.uniform(0, 1000, len(hz))
    near = np.arange(len(hz)) % 3 == 2
    pz = rs.choice([-1, 1], len(hz)) * np.where(near, 10 ** rs.uniform(-4, -2, len(hz)), rs.uniform(0.05, 0.5, len(hz)))
    Hd = H.astype(np.float64)
    x = (pz - Hd[2, 1] * y - Hd[2, 2]) / Hd[2, 0]
    a[hz] = np.stack([x, y], 1).astype(np.float32)
    ah = np.concatenate([a[hz].astype(np.float64), np.ones((len(hz), 1))], 1) @ Hd.T
    proj = ah[:, :2] / (ah[:, 2:] + 1e-8) + np.where(np.arange(len(hz))[:, None] % 3 == 1, 50.0, 0.0)
    b[hz] = np.where(near[:, None], a[hz], proj).astype(np.float32)
    a[count:] = np.nan
    b[count:] = np.nan
    fr = _frac(lib, a, b, H, thr, n_max=n_max, count=count)
    k = int(round(fr * count))
    c, lo, hi = R.inlier_count(H, a[:count], b[:count], thr)
    assert lo <= k <= hi, (k, c, lo, hi)
    # the horizon points are decided: the bound leaves at most a handful ambiguous
    assert hi - lo <= 20, (lo, hi)
    # count through ops with the n_max = count buffer: same fraction
    assert _frac(lib, a[:count].copy(), b[:count].copy(), H, thr) == fr
