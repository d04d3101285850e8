"""The float64 references of tests/fp64_refs.py checked on the host, before any GPU test leans on them: the fit against the
reference's goldens, the algebraic mean channel against the correlation volume it replaces, the crop-aware keep rule against
the frame-sized rule of test_tracker_gpu.test_tc_select_kernel_semantics, and the upsampling crop against plain slicing."""
import numpy as np
import pytest
import torch

from oracle import hfit_ref, raft_ref
import fp64_refs as R


@pytest.mark.parametrize("case", ["n4", "n500", "n4096", "degen"])
def test_fp64_fit_reproduces_the_hfit_goldens(golden_dir, case):
    """Same tolerances as the GPU fit tests hold the kernel to against these goldens (test_homography_gpu,
    test_kernels_gpu.test_hfit_vs_golden_and_oracle)."""
    g = np.load(golden_dir / "hfit.npz")
    a, b, w = (g[f"{case}_{k}"][0] for k in "abw")
    corners = np.array([[100, 80], [1800, 80], [1800, 1000], [100, 1000.0]])
    tol, tol_irls = (0.05, 0.2) if case != "degen" else (5.0, 5.0)
    H = R.fit(a, b, w)
    assert H.dtype == np.float64
    assert R.corner_err(H, g[f"{case}_qr_w"][0], corners) < tol
    assert R.corner_err(R.fit(a, b), g[f"{case}_qr_now"][0], corners) < tol
    assert R.corner_err(R.fit_irls(a, b, w, huber_k=2.0), g[f"{case}_irls_huber2"][0], corners) < tol
    if case not in ("n4", "degen"):
        assert R.corner_err(R.fit_irls(a, b, w), g[f"{case}_irls_l1"][0], corners) < tol_irls
        assert R.corner_err(R.fit_irls(a, b, w, huber_k=0.01), g[f"{case}_irls_huber001"][0], corners) < tol_irls


def test_fp64_fit_stays_float64_throughout():
    """oracle.hfit_ref promotes: float64 inputs give a float64 system, normalisation and solution (only kornia's sqrt(2) is a
    float32 constant, as in the kernel), and the fp64 fit of noise-free correspondences recovers H to fp64 precision."""
    rs = np.random.RandomState(3)
    Hgt = np.array([[1.02, 0.03, 12.0], [-0.02, 0.98, -7.0], [2e-5, -1e-5, 1.0]])
    a = np.stack([rs.uniform(100, 1800, 200), rs.uniform(80, 1000, 200)], 1)
    ah = np.concatenate([a, np.ones((200, 1))], 1) @ Hgt.T
    b = ah[:, :2] / ah[:, 2:]
    A, bb, T1, T2 = hfit_ref.build_system(torch.from_numpy(a)[None], torch.from_numpy(b)[None], torch.ones(1, 200,
                                                                                                             dtype=torch.float64))
    assert A.dtype == bb.dtype == T1.dtype == T2.dtype == torch.float64
    H = R.fit(a, b)
    # (kornia's from_homogeneous scales the normalised points by 1 / (1 + 1e-8), and H is divided by h33 + 1e-8: both are
    #  reference semantics and move the corners by ~1e-7 px; the kernel leaves the first one out)
    assert R.corner_err(H, Hgt, R.box_corners(a)) < 1e-6
    # float32 inputs of the same points would lose ~1e-4 px: the reference is not the fp32 path in disguise
    H32 = hfit_ref.find_homography_nonhomogeneous_QR(torch.from_numpy(a).float()[None], torch.from_numpy(b).float()[None])[0]
    assert H32.dtype == torch.float32


def test_fp64_residuals_vanish_at_the_least_squares_solution():
    """fp64_refs.residuals is A x - b of the normalised weighted system: at the fp64 least-squares solution A^T r = 0."""
    rs = np.random.RandomState(4)
    a = rs.uniform(0, 500, (300, 2))
    b = a + rs.normal(0, 2, (300, 2))
    w = rs.uniform(0.1, 1, 300)
    A, bb, T1, T2 = hfit_ref.build_system(torch.from_numpy(a)[None], torch.from_numpy(b)[None], torch.from_numpy(w)[None])
    sol = torch.linalg.lstsq(A[0], bb[0]).solution[:, 0].numpy()
    t1, t2 = T1[0].numpy(), T2[0].numpy()
    norm = (t1[0, 0], t1[0, 2], t1[1, 2], t2[0, 0], t2[0, 2], t2[1, 2])
    r, mag = R.residuals(a, b, w, sol, norm)
    # (the oracle's normalised points carry kornia's 1 / (1 + 1e-8) factor, fp64_refs.residuals -- like the kernel -- not)
    assert np.allclose(r, (A[0].numpy() @ sol - bb[0, :, 0].numpy()), rtol=0, atol=1e-7)
    assert np.abs(A[0].numpy().T @ r).max() < 1e-7            # (zero up to the same 1e-8 factor)
    assert np.all(mag >= np.abs(r))


@pytest.mark.parametrize("c", [64, 96])
def test_algebraic_mean_equals_the_volume_mean(c):
    """mean_q <f1[p], f2[q]> / sqrt(C) is raft_ref's vol0.mean(-1) (raft_ref.py:238) on the same pair."""
    g = torch.Generator().manual_seed(c)
    h, w = 5, 7
    f1 = torch.randn(1, c, h, w, generator=g, dtype=torch.float64)
    f2 = torch.randn(1, c, h, w, generator=g, dtype=torch.float64)
    vol0 = raft_ref.corr_pyramid(f1, f2, num_levels=1)[0]
    ref = vol0.view(1, h, w, -1).mean(dim=-1).reshape(-1).numpy()
    m = R.mean_channel(f1[0].reshape(c, -1).T, f2[0].reshape(c, -1).T)
    # (corr_pyramid divides by a float32 sqrt(C): exact for C = 64, one float32 rounding for 96)
    assert np.allclose(m, ref, rtol=1e-7 if c == 96 else 1e-13, atol=1e-13)


def test_wh_reduce_reference():
    g = torch.Generator().manual_seed(1)
    act = torch.randn(3, 5, 8, generator=g, dtype=torch.float64)
    w = torch.randn(8, generator=g, dtype=torch.float64)
    out, mag = R.wh_reduce(act, w, 0.25)
    want = [0.25 + sum(float(act[p, t] @ w) for t in range(5)) / 5 for p in range(3)]
    assert np.allclose(out, want, rtol=0, atol=1e-13) and np.all(mag > 0)


def test_upflow8_crop_is_the_sliced_full_upsampling():
    flow = torch.randn(1, 2, 3, 4, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    full = (8 * torch.nn.functional.interpolate(flow, size=(24, 32), mode="bilinear", align_corners=True))[0].numpy()
    assert np.array_equal(R.upflow8_crop(flow, (3, 5), 17, 22), full[:, 3:20, 5:27])
    assert np.array_equal(R.upflow8_crop(flow, (0, 0), 24, 32), full)


def _existing_rule(d, tmask, pw, h, w):
    """The rule of test_tracker_gpu.test_tc_select_kernel_semantics, verbatim (frame-sized flow grid, finite dst)."""
    keep = (tmask.reshape(-1) > 0) & ~((d[0] < 0) | (d[1] < 0) | (np.rint(d[0]) >= w) | (np.rint(d[1]) >= h))
    ri = np.clip(np.rint(d[1]).astype(np.int64), 0, h - 1) * w + np.clip(np.rint(d[0]).astype(np.int64), 0, w - 1)
    keep &= pw.reshape(-1)[ri] > 0
    return keep


@pytest.mark.parametrize("h,w", [(20, 30), (25, 24), (50, 40), (64, 33)])
def test_keep_rule_agrees_with_the_existing_rule(h, w):
    n = h * w
    rs = np.random.RandomState(n)
    tmask = (rs.uniform(size=(h, w)) < 0.97).astype(np.uint8) * 255
    d = np.stack([rs.uniform(-3, w + 3, n), rs.uniform(-3, h + 3, n)]).astype(np.float32)
    d[0, :40] = np.float32(w - 0.5)                       # rint half-way cases (to even) at the right / bottom edge
    d[1, 40:80] = np.float32(h - 0.5)
    pw = (rs.uniform(size=(h, w)) < 0.9).astype(np.uint8)
    assert np.array_equal(R.keep_rule(d, tmask, pw, h, w), _existing_rule(d, tmask, pw, h, w))
    # crop geometry: the grid is the top-left gh x gw of the frame; each grid pixel reads its own frame pixel of tmask
    gh, gw = h - 3, w - 5
    dg = d[:, :gh * gw]
    keep = R.keep_rule(dg, tmask, pw, gh, gw)
    full = _existing_rule(np.pad(dg.reshape(2, gh, gw), ((0, 0), (0, 3), (0, 5)), constant_values=-1).reshape(2, -1),
                          tmask, pw, h, w).reshape(h, w)
    assert np.array_equal(keep, full[:gh, :gw].reshape(-1))
    # NaN and infinite targets are out
    d2 = dg.copy()
    d2[0, :3] = [np.nan, np.inf, -np.inf]
    d2[1, 3:6] = [np.nan, np.inf, -np.inf]
    assert not R.keep_rule(d2, np.full((h, w), 255, np.uint8), None, gh, gw)[:6].any()


def test_sobol_ranks_match_the_reference_subsampler():
    from woft_amd import presets
    u = presets.sobol_points(500)
    for N in (0, 3, 499, 500, 501, 1000, 12345):
        mask = hfit_ref.sobol_subsample_mask(N, 500) if N > 0 else np.zeros(0, bool)
        assert np.array_equal(R.sobol_ranks(N, u), np.nonzero(mask)[0]), N
