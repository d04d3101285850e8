"""The backward of the weighted least-squares fit (`woft_hfit_batched_bwd`, csrc/hfit.hip `hfit_batched_bwd_kernel`: one
workgroup per element) and the autograd path of `find_homography_nonhomogeneous_QR` on top of it.

Shapes: N = 4 (exactly determined: zero residual, the true weight gradient is 0), 7 (part of one wave), 65 (one lane into the
second wave), 500 (the workload's size), 2048 (the limit: two correspondences per thread); B = 1 and 3.

Accuracy rule.  Reference: float64 torch autograd of the oracle (oracle/hfit_ref.py, torch.linalg.qr) on the same float32
inputs, for a full random gout; error of a gradient tensor = max |g - g64| / max |g64|, per batch element.  Yardstick: the same
oracle run in float32 through torch autograd on the CPU -- what a user has without this kernel -- on the same case.  The kernel's
error must not exceed 4 x that error, floor 1e-6: the factor is for a different summation order and for the fp32 row
construction, which both share in kind but not in order; the kernel accumulates in fp64.  The cases (tests/hfit_bwd_host.case:
points in [100, 1800] x [80, 1000], homography within 5 % of the identity, 0.5 px noise, 10 % outliers of 30 px, weights in
[0.05, 0.95]) are ones where the float32 oracle itself is within 1e-4 of float64 (asserted), so the yardstick means something;
N = 5 is left out (the float32 oracle is at 3e-3 there).  N = 4: gpa, gpb by the same rule; gw absolutely,
|gw| <= 1e-4 x max |gw64| of the N = 7 case.  Run with -s for the table of measured (kernel, float32 oracle) pairs.

Bit identity and isolation are compared as bytes, without a tolerance.  The NaN that some of these tests place beyond a count
or meet in a failed fit's H are values, not faults."""
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hfit_bwd_host as HB  # noqa: E402
import pytracking.utils.least_squares_H as L  # noqa: E402  (the shim's import path, as configs use it)
from oracle import hfit_ref  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
NS = (4, 7, 65, 500, 2048)
FACTOR, FLOOR, ORACLE32_MAX = 4.0, 1e-6, 1e-4
_REFS = {}
_TABLE = []


def _note(case, name, err, e32):
    _TABLE.append((case, name, err, e32))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for case, name, err, e32 in _TABLE:
        print(f"\n[hfit backward] {case} {name}: kernel {err:.3e}, float32 oracle {e32:.3e}")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from woft_amd import _lib
    _lib.load()
    return _lib


def _oracle(a, b, w, gout, dtype, loss=None):
    """Gradients of sum(gout * H) (or of loss(H)) through the oracle on the CPU in `dtype` -> float64 numpy [ga, gb(, gw)]."""
    ta, tb = (torch.tensor(x, dtype=dtype, requires_grad=True) for x in (a, b))
    tw = None if w is None else torch.tensor(w, dtype=dtype, requires_grad=True)
    H = hfit_ref.find_homography_nonhomogeneous_QR(ta, tb, tw)
    out = (H * torch.tensor(gout, dtype=dtype)).sum() if loss is None else loss(H, dtype)
    gs = torch.autograd.grad(out, [ta, tb] + ([] if tw is None else [tw]))
    return [g.double().numpy() for g in gs]


def _refs(n, batch, weighted=True):
    """The case (float32 numpy) and its float64 / float32 oracle gradients, computed once and shared."""
    key = (n, batch, weighted)
    if key not in _REFS:
        a, b, w, gout = HB.case(n, seed=100 + n, batch=batch)
        w = w if weighted else None
        _REFS[key] = (a, b, w, gout, _oracle(a, b, w, gout, torch.float64), _oracle(a, b, w, gout, torch.float32))
    return _REFS[key]


def _dev(x, grad=False):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t.requires_grad_() if grad else t


def _public(a, b, w, gout, grad=(True, True, True)):
    """find_homography_nonhomogeneous_QR on the device and H.backward(gout) -> (H, [a.grad, b.grad, w.grad] as numpy or None)."""
    ta, tb, tw = _dev(a, grad[0]), _dev(b, grad[1]), _dev(w, grad[2] and w is not None)
    H = L.find_homography_nonhomogeneous_QR(ta, tb, tw)
    H.backward(_dev(gout))
    torch.cuda.synchronize()
    return H.detach(), [None if (t is None or t.grad is None) else t.grad.cpu().numpy() for t in (ta, tb, tw)]


def _rel(g, g64):
    return float(np.abs(g.astype(np.float64) - g64).max() / np.abs(g64).max())


def _check_accuracy(case, got, g64, g32, gw_abs=None, oracle32_max=ORACLE32_MAX):
    """The accuracy rule on every element and tensor; gw_abs: the N = 4 bound on |gw| instead of the relative rule."""
    for name, g, r64, r32 in zip(("gpa", "gpb", "gw"), got, g64, g32):
        assert g is not None and g.shape == r64.shape and np.isfinite(g).all(), (case, name)
        for e in range(r64.shape[0]):
            if name == "gw" and gw_abs is not None:
                worst = float(np.abs(g[e]).max())
                _note(f"{case} e={e}", "max |gw| (true value 0)", worst, float(np.abs(r32[e]).max()))
                assert worst <= gw_abs, (case, e, worst, gw_abs)
                continue
            err, e32 = _rel(g[e], r64[e]), _rel(r32[e], r64[e])
            _note(f"{case} e={e}", name, err, e32)
            assert e32 <= oracle32_max, f"{case} e={e} {name}: the float32 oracle is {e32:.3e} from float64: no yardstick"
            assert err <= max(FACTOR * e32, FLOOR), f"{case} e={e} {name}: kernel {err:.3e}, float32 oracle {e32:.3e}"


def _gw_scale_n7():
    return float(np.abs(_refs(7, 1)[4][2]).max())


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", [1, 3])
def test_forward_is_unchanged_by_the_graph(B, N):
    a, b, w, _, _, _ = _refs(N, B)
    with torch.no_grad():
        H0 = L.find_homography_nonhomogeneous_QR(_dev(a), _dev(b), _dev(w))
    H1 = L.find_homography_nonhomogeneous_QR(_dev(a, True), _dev(b, True), _dev(w, True))
    assert H1.requires_grad and not H0.requires_grad and bool(torch.isfinite(H0).all())
    assert torch.equal(H1.detach(), H0)
    H2 = L.find_homography_nonhomogeneous_QR(_dev(a), _dev(b), _dev(w, True))          # only the weights want a gradient
    assert H2.requires_grad and torch.equal(H2.detach(), H0)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", [1, 3])
def test_gradients_against_float64_autograd_of_the_oracle(B, N):
    a, b, w, gout, g64, g32 = _refs(N, B)
    _, got = _public(a, b, w, gout)
    _check_accuracy(f"N={N} B={B}", got, g64, g32, gw_abs=1e-4 * _gw_scale_n7() if N == 4 else None)


@pytest.mark.parametrize("N", NS)
def test_weights_none(N):
    a, b, _, gout, g64, g32 = _refs(N, 1, weighted=False)
    H, got = _public(a, b, None, gout)
    assert got[2] is None and len(g64) == 2
    _check_accuracy(f"N={N} B=1 unweighted", got[:2], g64, g32)


@pytest.mark.parametrize("N", NS)
def test_batch_element_has_the_bits_of_its_solo_run(N):
    a, b, w, gout, _, _ = _refs(N, 3)
    _, full = _public(a, b, w, gout)
    for e in range(3):
        _, solo = _public(a[e:e + 1], b[e:e + 1], w[e:e + 1], gout[e:e + 1])
        for name, f, s in zip(("gpa", "gpb", "gw"), full, solo):
            assert f[e].tobytes() == s[0].tobytes(), (N, e, name)


@pytest.mark.parametrize("N", NS)
def test_skipped_gradients_leave_the_others_their_bits(N):
    a, b, w, gout, _, _ = _refs(N, 3)
    _, full = _public(a, b, w, gout)
    for grad in ((False, False, True), (True, False, False), (False, True, True)):
        _, part = _public(a, b, w, gout, grad=grad)
        for name, want, f, p in zip(("gpa", "gpb", "gw"), grad, full, part):
            if want:
                assert p is not None and p.tobytes() == f.tobytes(), (N, grad, name)
            else:
                assert p is None, (N, grad, name)


def _raw(lib, a, b, w, gout, counts=None, want=(True, True, True)):
    """One woft_hfit_batched_bwd call on (B, n_max, ...) numpy operands -> (gpa, gpb, gw as numpy or None, status list);
    the outputs start as 777 everywhere."""
    from woft_amd import ops
    pa, pb, pw, g = _dev(a), _dev(b), _dev(w), _dev(gout.reshape(-1, 9))
    B, n = a.shape[0], a.shape[1]
    gpa = torch.full((B, n, 2), 777.0, device="cuda") if want[0] else None
    gpb = torch.full((B, n, 2), 777.0, device="cuda") if want[1] else None
    gw = torch.full((B, n), 777.0, device="cuda") if want[2] else None
    st = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda")
    ops.hfit_batched_bwd(pa, pb, pw, g, gpa, gpb, gw, status=st, counts=cnt)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in (gpa, gpb, gw)], [int(s) for s in st.cpu().numpy()]


@pytest.mark.parametrize("N", [7, 65, 500, 2048])
def test_ragged_batch_at_the_abi(lib, N):
    """counts = (4, N, N - 1) with NaN in every row beyond the count: the tail gets exact zeros, the head is finite and has the
    bytes of the call on the first count rows alone (n_max = count, no counts)."""
    counts = (4, N, N - 1)
    a, b, w, gout, _, _ = _refs(N, 3)
    a, b, w = a.copy(), b.copy(), w.copy()
    for e, c in enumerate(counts):
        a[e, c:], b[e, c:], w[e, c:] = np.nan, np.nan, np.nan
    got, st = _raw(lib, a, b, w, gout, counts=counts)
    assert st == [0, 0, 0]
    for e, c in enumerate(counts):
        solo, ss = _raw(lib, a[e:e + 1, :c], b[e:e + 1, :c], w[e:e + 1, :c], gout[e:e + 1])
        assert ss == [0]
        for name, g, s in zip(("gpa", "gpb", "gw"), got, solo):
            assert np.isfinite(g[e, :c]).all() and (name == "gw" or np.abs(g[e, :c]).max() > 0), (N, e, name)
            assert g[e, :c].tobytes() == s[0].tobytes(), (N, e, name)
            assert g[e, c:].tobytes() == np.zeros_like(g[e, c:]).tobytes(), (N, e, name)      # exact +0.0, not 777, not NaN


def test_failing_elements_get_zero_gradients_and_leave_their_neighbour_alone(lib):
    """Element 0 good; element 1 all points identical (power-of-two coordinates: the normalised points are exactly 0, the Gram
    matrix has a zero pivot: status 2); element 2 with counts = 3 (status 1)."""
    N = 65
    a, b, w, gout, _, _ = _refs(N, 3)
    a, b = a.copy(), b.copy()
    a[1], b[1] = np.float32([512.0, 256.0]), np.float32([1024.0, 128.0])
    counts = (N, N, 3)
    for want in ((True, True, True), (False, False, True)):
        got, st = _raw(lib, a, b, w, gout, counts=counts, want=want)
        assert st == [0, 2, 1]
        solo, ss = _raw(lib, a[:1], b[:1], w[:1], gout[:1], want=want)
        assert ss == [0]
        for name, g, s in zip(("gpa", "gpb", "gw"), got, solo):
            if g is None:
                continue
            assert g[0].tobytes() == s[0].tobytes() and np.isfinite(g[0]).all() and np.abs(g[0]).max() > 0, name
            for e in (1, 2):
                assert g[e].tobytes() == np.zeros_like(g[e]).tobytes(), (name, e)
    # the public estimator: the failed element's H is NaN (the forward's report), its gradients are zeros, not NaN
    ta, tb, tw = _dev(a[:2], True), _dev(b[:2], True), _dev(w[:2], True)
    H = L.find_homography_nonhomogeneous_QR(ta, tb, tw)
    assert bool(torch.isnan(H[1]).all()) and bool(torch.isfinite(H[0]).all())
    H.backward(torch.ones_like(H))
    for t in (ta, tb, tw):
        assert bool((t.grad[1] == 0).all()) and bool(torch.isfinite(t.grad[0]).all()) and float(t.grad[0].abs().max()) > 0


def _training_config():
    sys.dont_write_bytecode = True
    path = ROOT / "tests" / "configs" / "training_forms.py"
    m = types.ModuleType("training_config_bwd")
    m.__file__ = str(path)
    exec(compile(path.read_text(), str(path), "exec"), m.__dict__)
    return m.get_config()


GT_H = np.array([[1.02, 0.03, 12.0], [-0.02, 0.98, -7.0], [2e-5, -1e-5, 1.0]])


def _reproj_loss(gt, pts):
    """mean of torch_reproj_errors(GT_H, H, pts), restated on the CPU in the dtype asked for (float64: the reference)."""
    def loss(H, dtype):
        G, P = torch.tensor(gt, dtype=dtype), torch.tensor(pts, dtype=dtype)
        q = torch.linalg.inv(H) @ (G @ torch.cat([P, torch.ones_like(P[:, :1])], dim=1))
        z = q[:, 2:3]
        rp = torch.where(z.abs() > 1e-8, 1.0 / (z + 1e-8), torch.ones_like(z)) * q[:, :2]
        return torch.sqrt(torch.square(rp - P).sum(dim=1)).mean()
    return loss


def test_training_form_loss_reaches_the_weights():
    """loss = conf.train.loss_fn(GT_H, conf.train.H_estimator(a, b, w), pts).mean() on the device; w.grad (and the point
    gradients) against the float64 end-to-end autograd of the oracle plus a float64 restatement of the loss, by the accuracy
    rule with the float32 end-to-end autograd on the CPU as the yardstick.  The loss is taken at 16 points of a 16-px box, the
    regime the float32 error helpers are specified for (tests/test_hfit_batched_gpu.py): at the correspondences' own 1e3-px
    coordinates the float32 loss alone puts 1e-3 of noise on these gradients, on the CPU and on the device alike, and the
    comparison would say nothing about the fit (here the float32 yardstick is 6e-6 / 5e-6 / 6e-5 on gpa / gpb / gw; it is held
    to 2e-4).  A non-contiguous w gets its gradient in its layout."""
    conf = _training_config()
    N, B = 500, 3
    a, b, w, _, _, _ = _refs(N, B)
    gt = np.tile(GT_H[None], (B, 1, 1)).astype(np.float32)
    pts = np.random.RandomState(5).uniform(0.0, 16.0, (B, 2, 16)).astype(np.float32)
    g64 = _oracle(a, b, w, None, torch.float64, loss=_reproj_loss(gt, pts))
    g32 = _oracle(a, b, w, None, torch.float32, loss=_reproj_loss(gt, pts))

    def run(tw):
        ta, tb = _dev(a, True), _dev(b, True)
        loss = conf.train.loss_fn(_dev(gt), conf.train.H_estimator(ta, tb, tw), _dev(pts)).mean()
        assert loss.requires_grad and bool(torch.isfinite(loss))
        loss.backward()
        torch.cuda.synchronize()
        return [t.grad.cpu().numpy() for t in (ta, tb)] + [tw.grad]
    tw = _dev(w, True)
    got = run(tw)
    wgrad = got[2]
    got[2] = wgrad.cpu().numpy()
    _check_accuracy(f"training form N={N} B={B}", got, g64, g32, oracle32_max=2e-4)
    # a transposed view as the weight leaf
    tn = torch.from_numpy(np.ascontiguousarray(w.T)).cuda().t().requires_grad_()
    assert not tn.is_contiguous() and tn.is_leaf and tuple(tn.shape) == (B, N)
    gn = run(tn)[2]
    assert tuple(gn.shape) == (B, N) and torch.equal(gn, wgrad)


def test_irls_is_still_forward_only():
    a, b, w, _, _, _ = _refs(500, 3)
    tw = _dev(w, True)
    H = L.find_homography_IRLSq_QR(_dev(a), _dev(b), tw)
    assert not H.requires_grad and H.grad_fn is None and bool(torch.isfinite(H).all())
    H = L.find_homography_IRLSq_QR(_dev(a), _dev(b), tw, reweighting_fn=lambda r: 1.0 / (1.0 + (r / 0.02) ** 2), n_iter=2)
    assert not H.requires_grad
