"""The batched homography fit (`woft_hfit_batched`, csrc/hfit.hip `hfit_batched_kernel`: one workgroup per batch element,
the body of the one-workgroup `hfit_kernel`) and what the public estimators do with it.

The kernel's contract is bit identity with `woft_hfit` (ws = NULL) on each element alone, so every comparison of fits here is
a comparison of bytes (NaN outputs included): no tolerance.  tests/golden/hfit.npz holds no two reference cases of equal N
(4, 500, 4096, 300), so the golden check stacks the n500 case with its row-reversed, unit-weight copy -- the batch of
test_homography_gpu.test_batch_of_two -- and applies that test's bounds to every element.

Projection-error helpers: float32 on the device against a float64 numpy restatement kept here, with the tolerance of the
existing torch_proj_errors test (tests/test_homography_gpu.py: rtol 1e-5, atol 1e-4).  The case is small and well conditioned
on purpose: points in [0, 16]^2, homographies within 5 % of the identity with at most half a pixel of translation (condition
number below 2).  A float32 evaluation of inv(E) G p, the division by z and the difference to the point is about a dozen
roundings of 2^-24 relative to values of size <= 20, amplified by the condition number of the inverted matrix: below
12 * 2^-24 * 20 * 2 = 3e-5 px whatever the order of the operations -- inside the absolute term.  float32 rounds relative to the
coordinate: the same formula, bit-identical to the reference's own float32 result on the host, is 1.8e-4 px from float64 at
64-px coordinates with 4-px translations, and about 1e-3 px at 2e3, so that absolute term cannot be met there by any float32
evaluation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pytracking.utils.least_squares_H as L  # noqa: E402  (the shim's import path, as configs use it)

RTOL, ATOL = 1e-5, 1e-4
LSQ, L1, HUBER = 0, 1, 2
# (reweight, huber_k, n_irls): the three losses with and without passes; Huber k = 1 never bites on Hartley-normalised
# residuals, so k = 0.01 is run too
MODES = [(LSQ, 1.0, 0), (LSQ, 1.0, 5), (L1, 1.0, 0), (L1, 1.0, 5), (HUBER, 1.0, 0), (HUBER, 1.0, 5), (HUBER, 0.01, 5)]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from woft_amd import _lib
    _lib.load()
    return _lib


def _batch(B, N, seed):
    """Seeded correspondences under a random, well-conditioned homography per element, plus 0.3 px noise:
    numpy float32 a, b (B, N, 2), w (B, N)."""
    rs = np.random.RandomState(seed)
    a = np.stack([rs.uniform(100, 1800, (B, N)), rs.uniform(80, 1000, (B, N))], -1)
    if N < 8:                                    # few points: spread them over the corners of the box, in general position
        cx = np.array([200.0, 1700.0, 1600.0, 150.0, 900.0, 500.0, 1300.0])[:N]
        cy = np.array([100.0, 180.0, 950.0, 900.0, 500.0, 300.0, 700.0])[:N]
        a = np.stack([cx, cy], -1)[None] + rs.uniform(-40, 40, (B, N, 2))
    H = np.eye(3)[None] + rs.uniform(-1, 1, (B, 3, 3)) * np.array([[0.05, 0.05, 20.0], [0.05, 0.05, 20.0], [2e-5, 2e-5, 0.0]])
    ah = np.concatenate([a, np.ones((B, N, 1))], -1) @ H.transpose(0, 2, 1)
    b = ah[..., :2] / ah[..., 2:] + rs.normal(0, 0.3, (B, N, 2))
    w = rs.uniform(0.05, 1.0, (B, N))
    return a.astype(np.float32), b.astype(np.float32), w.astype(np.float32)


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _single(lib, pa, pb, w, n_max, count=None, reweight=0, huber_k=1.0, n_irls=0):
    """woft_hfit with ws = NULL (the one-workgroup kernel) on one element -> (36 bytes of H, status)."""
    Hd = torch.full((9,), 777.0, device="cuda")
    st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    lib.check(lib.load().woft_hfit(pa.data_ptr(), pb.data_ptr(), lib.ptr(w), n_max, lib.ptr(cnt), reweight, float(huber_k),
                                   n_irls, None, Hd.data_ptr(), st.data_ptr(), lib.stream_ptr()), "woft_hfit")
    torch.cuda.synchronize()
    return Hd.cpu().numpy().tobytes(), int(st.item())


def _batched(pa, pb, w, counts=None, reweight=0, huber_k=1.0, n_irls=0):
    """One woft_hfit_batched call -> ([36 bytes of H per element], [status per element])."""
    from woft_amd import ops
    B = pa.shape[0]
    Hd = torch.full((B, 9), 777.0, device="cuda")
    st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda")
    ops.hfit_batched(pa, pb, w, Hd, st, counts=cnt, reweight=reweight, huber_k=huber_k, n_irls=n_irls)
    torch.cuda.synchronize()
    Hn = Hd.cpu().numpy()
    return [Hn[b].tobytes() for b in range(B)], [int(s) for s in st.cpu().numpy()]


def _h(raw):
    return np.frombuffer(raw, np.float32)


@pytest.mark.parametrize("N", [4, 7, 500, 2048])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_bit_identity_with_the_single_fit(lib, B, N):
    a, b, w = _batch(B, N, seed=1000 * B + N)
    pa, pb, pw = _dev(a), _dev(b), _dev(w)
    for weights in (pw, None):
        for reweight, k, n_irls in MODES:
            kw = dict(reweight=reweight, huber_k=k, n_irls=n_irls)
            Hb, sb = _batched(pa, pb, weights, **kw)
            for e in range(B):
                Hs, ss = _single(lib, pa[e], pb[e], None if weights is None else weights[e], N, **kw)
                what = (B, N, weights is not None, reweight, k, n_irls, e)
                assert sb[e] == ss, what
                assert Hb[e] == Hs, (what, _h(Hb[e]), _h(Hs))
                if reweight == LSQ:
                    assert ss == 0 and np.all(np.isfinite(_h(Hs))), what       # (the comparison is of real fits)


@pytest.mark.parametrize("N", [7, 500, 2048])
def test_ragged_batch(lib, N):
    """counts = [N, 4, 3, 0, N - 1]: rows beyond counts[b] are NaN and never read; too few points -> woft_hfit's status."""
    counts = [N, 4, 3, 0, N - 1]
    a, b, w = _batch(5, N, seed=77 + N)
    for e, c in enumerate(counts):
        a[e, c:], b[e, c:], w[e, c:] = np.nan, np.nan, np.nan
    pa, pb, pw = _dev(a), _dev(b), _dev(w)
    for weights in (pw, None):
        for reweight, k, n_irls in ((LSQ, 1.0, 0), (L1, 1.0, 5), (HUBER, 0.01, 5)):
            kw = dict(reweight=reweight, huber_k=k, n_irls=n_irls)
            Hb, sb = _batched(pa, pb, weights, counts=counts, **kw)
            for e, c in enumerate(counts):
                we = None if weights is None else weights[e]
                if c >= 1:       # the single fit on the first c rows alone: it never sees the NaN tail
                    Hs, ss = _single(lib, pa[e, :c].contiguous(), pb[e, :c].contiguous(),
                                     None if we is None else we[:c].contiguous(), c, **kw)
                else:
                    Hs, ss = _single(lib, pa[e], pb[e], we, N, count=0, **kw)
                assert (sb[e], Hb[e]) == (ss, Hs), (N, e, c, reweight, _h(Hb[e]), _h(Hs))
                if c < 4:
                    assert ss == 1 and np.all(np.isnan(_h(Hb[e])))
                elif reweight == LSQ:
                    assert ss == 0 and np.all(np.isfinite(_h(Hb[e])))
    # counts above n_max are clamped to n_max, as woft_hfit clamps its count
    a, b, w = _batch(2, N, seed=5)
    pa, pb, pw = _dev(a), _dev(b), _dev(w)
    assert _batched(pa, pb, pw, counts=[N + 9, N]) == _batched(pa, pb, pw)


def test_failing_elements_leave_their_neighbours_alone(lib):
    N = 500
    a, b, w = _batch(5, N, seed=31)
    t = np.arange(N, dtype=np.float32)
    a[1] = np.stack([100 + 3 * t, 80 + 1.5 * t], -1)                  # element 1: every point on one line
    b[1] = a[1] + np.float32([5.0, -3.0])
    a[3, 250, 1] = np.nan                                             # element 3: one NaN coordinate
    pa, pb, pw = _dev(a), _dev(b), _dev(w)
    good = [0, 2, 4]
    ga, gb, gw = (x[good].contiguous() for x in (pa, pb, pw))
    for reweight, k, n_irls in ((LSQ, 1.0, 0), (L1, 1.0, 5), (HUBER, 0.01, 5)):
        kw = dict(reweight=reweight, huber_k=k, n_irls=n_irls)
        Hb, sb = _batched(pa, pb, pw, **kw)
        for e in (1, 3):
            Hs, ss = _single(lib, pa[e], pb[e], pw[e], N, **kw)
            assert (sb[e], Hb[e]) == (ss, Hs), (e, reweight, sb[e], ss, _h(Hb[e]), _h(Hs))
        assert sb[3] == 2 and np.all(np.isnan(_h(Hb[3])))            # non-finite input: the singular-system status
        Hg, sg = _batched(ga, gb, gw, **kw)
        for i, e in enumerate(good):
            assert (sb[e], Hb[e]) == (sg[i], Hg[i]) and sb[e] == 0, (e, reweight)


def _noncontiguous(x):
    """(B, N, 2) -> the same values as a transposed view of a (B, 2, N) tensor."""
    v = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert not v.is_contiguous() and torch.equal(v, x)
    return v


def test_public_estimators_batch_equals_stacked_single_calls():
    a, b, w = (_dev(x) for x in _batch(3, 500, seed=9))
    an, bn, wn = _noncontiguous(a), _noncontiguous(b), w.t().contiguous().t()
    assert not wn.is_contiguous()
    huber = lambda r: L.IRLSq_Huber(r, k=0.01)
    cauchy = lambda r: 1.0 / (1.0 + (r / 0.02) ** 2)
    fits = {"qr": lambda x, y, ww: L.find_homography_nonhomogeneous_QR(x, y, ww),
            "irls l1": lambda x, y, ww: L.find_homography_IRLSq_QR(x, y, ww),
            "irls huber": lambda x, y, ww: L.find_homography_IRLSq_QR(x, y, ww, reweighting_fn=huber),
            "irls lambda": lambda x, y, ww: L.find_homography_IRLSq_QR(x, y, ww, reweighting_fn=cauchy, n_iter=4)}
    for name, fit in fits.items():
        for ww, wwn in ((w, wn), (None, None)):
            H = fit(an, bn, wwn)
            assert tuple(H.shape) == (3, 3, 3) and H.is_cuda and H.dtype == torch.float32
            single = torch.cat([fit(a[e:e + 1], b[e:e + 1], None if ww is None else ww[e:e + 1]) for e in range(3)], 0)
            assert bool(torch.isfinite(H).all()) and torch.equal(H, single), (name, ww is not None)
            assert torch.equal(fit(a, b, ww), H)                              # contiguous operands: the same bits
    # host tensors in, host tensor out (the QR estimator takes them; the IRLS one asserts device tensors)
    Hc = L.find_homography_nonhomogeneous_QR(an.cpu(), bn.cpu(), wn.cpu())
    assert not Hc.is_cuda and torch.equal(Hc, L.find_homography_nonhomogeneous_QR(a, b, w).cpu())
    with pytest.raises(AssertionError):
        L.find_homography_IRLSq_QR(a.cpu(), b.cpu(), w.cpu())
    with pytest.raises(AssertionError):                                        # weights of another length
        L.find_homography_nonhomogeneous_QR(a, b, w[:, :-1])


def _corner_err(Ha, Hb):
    """As test_homography_gpu._corner_err: the largest corner displacement between two homographies, in pixels."""
    c = np.array([[100, 80, 1], [1800, 80, 1], [1800, 1000, 1], [100, 1000, 1.0]]).T
    pa, pb = np.asarray(Ha, np.float64) @ c, np.asarray(Hb, np.float64) @ c
    return np.abs(pa[:2] / pa[2] - pb[:2] / pb[2]).max()


def test_golden_cases_stacked(golden_dir):
    g = np.load(golden_dir / "hfit.npz")
    a, b, w = (torch.from_numpy(g[f"n500_{k}"]).cuda() for k in "abw")
    a3, b3 = torch.cat([a, a.flip(1), a], 0), torch.cat([b, b.flip(1), b], 0)
    w3 = torch.cat([w, torch.ones_like(w), w], 0)
    H = L.find_homography_nonhomogeneous_QR(a3, b3, w3).cpu().numpy()
    assert _corner_err(H[0], g["n500_qr_w"][0]) < 0.05 and _corner_err(H[2], g["n500_qr_w"][0]) < 0.05
    assert _corner_err(H[1], g["n500_qr_now"][0]) < 0.05                       # unit weights, permuted rows
    H = L.find_homography_IRLSq_QR(a3, b3, w3, reweighting_fn=lambda r: L.IRLSq_Huber(r, k=2)).cpu().numpy()
    assert _corner_err(H[0], g["n500_irls_huber2"][0]) < 0.05 and _corner_err(H[2], g["n500_irls_huber2"][0]) < 0.05
    H = L.find_homography_IRLSq_QR(a3, b3, w3).cpu().numpy()
    assert _corner_err(H[0], g["n500_irls_l1"][0]) < 0.2 and _corner_err(H[2], g["n500_irls_l1"][0]) < 0.2


@pytest.mark.parametrize("B,N", [(1, 500), (1, 3000), (2, 2049)])
def test_other_shapes_take_the_single_fit_path(B, N):
    """B == 1, and N above the one-workgroup limit at any B, are served by ops.hfit per element as before."""
    from woft_amd import ops
    a, b, w = (_dev(x) for x in _batch(B, N, seed=N))
    for kw in (dict(), dict(reweight=L1, n_irls=5)):
        H = L.find_homography_nonhomogeneous_QR(a, b, w) if not kw else L.find_homography_IRLSq_QR(a, b, w)
        for e in range(B):
            Hd, st = torch.zeros(9, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
            ops.hfit(a[e], b[e], w[e], Hd, st, **kw)
            assert int(st.item()) == 0 and torch.equal(H[e].reshape(9), Hd), (B, N, kw)


# ---- projection-error helpers ---------------------------------------------------------------------------------------------
def _p2e64(h):
    z = h[:, 2:3]
    with np.errstate(divide="ignore"):
        sc = np.where(np.abs(z) > 1e-8, 1.0 / (z + 1e-8), 1.0)
    return sc * h[:, :2]


def _e2p64(p):
    return np.concatenate([p, np.ones_like(p[:, :1])], 1)


def _helper_case():
    rs = np.random.RandomState(41)
    scale = np.array([[0.05, 0.05, 0.5], [0.05, 0.05, 0.5], [2e-4, 2e-4, 0.0]])[None]
    gt = np.eye(3)[None] + scale * rs.uniform(-1, 1, (4, 3, 3))
    est = gt + 0.5 * scale * rs.uniform(-1, 1, (4, 3, 3))
    pts = rs.uniform(0.0, 16.0, (4, 2, 16))
    return tuple(x.astype(np.float32) for x in (gt, est, pts))


def test_error_helpers_against_float64():
    gt, est, pts = _helper_case()
    G, E, P = _dev(gt), _dev(est), _dev(pts)
    g64, e64, p64 = (x.astype(np.float64) for x in (gt, est, pts))
    fwd = _p2e64(g64 @ _e2p64(p64))
    ref = {"torch_e2p": _e2p64(p64), "torch_p2e": fwd, "torch_H_proj": fwd,
           "torch_reproj_errors": np.sqrt(((_p2e64(np.linalg.inv(e64) @ (g64 @ _e2p64(p64))) - p64) ** 2).sum(1)),
           "torch_proj_diff_errors": np.sqrt(((fwd - _p2e64(e64 @ _e2p64(p64))) ** 2).sum(1))}
    got = {"torch_e2p": L.torch_e2p(P), "torch_p2e": L.torch_p2e(torch.matmul(G, L.torch_e2p(P))),
           "torch_H_proj": L.torch_H_proj(G, P), "torch_reproj_errors": L.torch_reproj_errors(G, E, P),
           "torch_proj_diff_errors": L.torch_proj_diff_errors(G, E, P)}
    for name, v in got.items():
        assert v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == ref[name].shape, name
        err = float(np.abs(v.cpu().numpy().astype(np.float64) - ref[name]).max())
        print(f"[error helpers] {name}: max |float32 on device - float64| = {err:.3e}")
        assert np.allclose(v.cpu().numpy(), ref[name], rtol=RTOL, atol=ATOL), (name, err)
    assert tuple(got["torch_reproj_errors"].shape) == (4, 16)
    assert float(ref["torch_reproj_errors"].min()) > 10 * ATOL and float(ref["torch_proj_diff_errors"].min()) > 10 * ATOL
    # the numpy helper: one pair, float64, plain division by z after normalising the composed homography
    for e in range(4):
        Hfb = np.linalg.inv(e64[e]) @ g64[e]
        q = Hfb @ np.vstack([p64[e], np.ones(16)])
        want = np.sqrt(((q[:2] / q[2:] - p64[e]) ** 2).sum(0))
        assert np.allclose(L.reproj_errors(g64[e], e64[e], p64[e], mean=False), want, rtol=1e-9, atol=0)
        assert np.isclose(L.reproj_errors(g64[e], e64[e], p64[e]), want.mean(), rtol=1e-9, atol=0)
    # z == 0: the conversion leaves the coordinates unscaled (the rule torch_proj_errors follows)
    h = torch.tensor([[[2.0, 4.0], [6.0, 8.0], [0.0, 2.0]]], device="cuda")
    assert torch.equal(L.torch_p2e(h).cpu(), torch.tensor([[[2.0, 4.0 / (2.0 + 1e-8)], [6.0, 8.0 / (2.0 + 1e-8)]]]))


def test_error_helpers_reproduce_the_reference_fixture_on_the_device(golden_dir):
    g = np.load(golden_dir / "reproj_errors.npz")
    G, E, P = (_dev(g[k]) for k in ("GT_H", "est_H", "pts"))
    got = {"torch_reproj_errors": L.torch_reproj_errors(G, E, P), "torch_proj_diff_errors": L.torch_proj_diff_errors(G, E, P),
           "torch_H_proj": L.torch_H_proj(G, P), "torch_e2p": L.torch_e2p(P),
           "torch_p2e": L.torch_p2e(torch.matmul(G, L.torch_e2p(P)))}
    for name, v in got.items():
        err = float(np.abs(v.cpu().numpy().astype(np.float64) - g[name]).max())
        print(f"[reproj fixture, device] {name}: max |diff| {err:.3e}")
        assert v.is_cuda and np.allclose(v.cpu().numpy(), g[name], rtol=RTOL, atol=ATOL), (name, err)
