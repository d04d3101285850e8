"""CPU checks of the differentiable weighted least-squares fit (no GPU).

1. The formulas the backward kernel implements (csrc/hfit.hip `hfit_bwd_one`), restated in float64
   numpy in tests/hfit_bwd_host.py, agree with float64 torch autograd of the oracle's find_homography_nonhomogeneous_QR
   (torch.linalg.qr, the path the reference trains through).  Tolerance 1e-7 of the largest entry of each gradient tensor: both
   sides are float64 (rounding ~1e-13 at these condition numbers); what separates them is the oracle's from_homogeneous, which
   scales the normalised points by 1 / (1 + 1e-8) -- exactly 1 in float32, where the kernel lives -- a relative 1e-8 on the
   points and a few of them on the gradients (measured 0.2e-8 .. 4e-8).  At N = 4 the system is exactly determined, the residual
   is 0 and so is the true weight gradient: it is compared absolutely, against the weight gradient scale of the N = 7 case.
2. `woft_hfit_batched_bwd` is declared, listed and exported, the ABI version stays 400, and every bad-argument case returns
   WOFT_EINVAL before any launch (host addresses, no device here).
3. N above the one-workgroup limit with a gradient requested raises NotImplementedError before any device work."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import hfit_bwd_host as HB
from oracle import hfit_ref

ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-7


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _oracle_grads(a, b, w, gout):
    """float64 torch.autograd.grad of sum(gout * H) through the oracle; a, b (1, N, 2), w (1, N) or None, gout (1, 3, 3)."""
    ta = torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    tw = None if w is None else torch.tensor(w, dtype=torch.float64, requires_grad=True)
    H = hfit_ref.find_homography_nonhomogeneous_QR(ta, tb, tw)
    ins = [ta, tb] + ([] if tw is None else [tw])
    gs = torch.autograd.grad((H * torch.tensor(gout, dtype=torch.float64)).sum(), ins)
    return [g[0].numpy() for g in gs], H[0].detach().numpy()


@pytest.fixture(scope="module")
def gw_scale_n7():
    a, b, w, gout = HB.case(7, seed=107)
    return float(np.abs(_oracle_grads(a, b, w, gout)[0][2]).max())


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("n", [4, 7, 65, 500])
def test_restatement_agrees_with_float64_autograd_of_the_oracle(n, weighted, gw_scale_n7):
    a, b, w, gout = HB.case(n, seed=100 + n)
    w = w if weighted else None
    ref, Href = _oracle_grads(a, b, w, gout)
    assert np.abs(HB.forward(a[0], b[0], None if w is None else w[0]) - Href).max() <= TOL * np.abs(Href).max()
    got = HB.backward(a[0], b[0], None if w is None else w[0], gout[0])
    assert (got[2] is None) == (w is None)
    for name, g, r in zip(("gpa", "gpb", "gw"), got, ref):
        assert g.shape == r.shape, name
        if name == "gw" and n == 4:
            err = float(np.abs(g).max())
            print(f"[hfit backward, host] N={n} {name}: max |gw| {err:.3e} (true value 0; N = 7 scale {gw_scale_n7:.3e})")
            assert err <= TOL * gw_scale_n7 and float(np.abs(r).max()) <= TOL * gw_scale_n7
            continue
        err = float(np.abs(g - r).max() / np.abs(r).max())
        print(f"[hfit backward, host] N={n} weighted={weighted} {name}: {err:.3e} of the largest entry")
        assert err <= TOL, (n, weighted, name, err)


def test_backward_exported_and_declared(lib):
    from woft_amd import _lib
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    assert "woft_hfit_batched_bwd" in declared and "woft_hfit_batched_bwd" in _lib.EXPORTS
    raw = ctypes.CDLL(str(ROOT / "woft_amd" / "lib" / "libwoft_hip.so"))
    assert hasattr(raw, "woft_hfit_batched_bwd")
    assert "least_squares_H.py:142-210" in header[header.index("Backward of the plain weighted fit"):header.index("int woft_hfit_batched_bwd")]
    assert lib.woft_abi_version() == 400                          # (an addition only: the version stays)


def test_backward_rejects_bad_arguments_without_a_launch(lib):
    """NULL pa / pb / gH, all three outputs NULL, gw with a NULL w, batch < 1 or above the bound, n_max < 1 or above
    WOFT_HFIT_SINGLE_MAX -> WOFT_EINVAL.  The non-NULL pointers are host addresses that no launch may see: there is no device
    here, the call must return first."""
    from woft_amd import ops
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok = dict(pa=p, pb=p, w=p, batch=2, n_max=4, counts=None, gH=p, gpa=p, gpb=p, gw=p, status=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.woft_hfit_batched_bwd(a["pa"], a["pb"], a["w"], a["batch"], a["n_max"], a["counts"], a["gH"], a["gpa"],
                                         a["gpb"], a["gw"], a["status"], None)
    for bad in (dict(pa=None), dict(pb=None), dict(gH=None), dict(gpa=None, gpb=None, gw=None), dict(w=None),
                dict(w=None, gpa=None, gpb=None), dict(batch=0), dict(batch=-3), dict(batch=ops.HFIT_BATCH_MAX + 1),
                dict(n_max=0), dict(n_max=-1), dict(n_max=ops.HFIT_SINGLE_MAX + 1)):
        assert call(**bad) == -1, bad
    assert lib.woft_hfit_batched_bwd(None, None, None, 1, 4, None, None, None, None, None, None, None) == -1


def test_gradient_above_the_one_workgroup_limit_is_refused_before_any_device_work():
    import pytracking.utils.least_squares_H as L
    from woft_amd import ops
    n = ops.HFIT_SINGLE_MAX + 1
    rs = np.random.RandomState(0)
    a = torch.from_numpy(rs.uniform(0, 1000, (1, n, 2)).astype(np.float32))
    b = a + 3.0
    w = torch.from_numpy(rs.uniform(0.1, 1.0, (1, n)).astype(np.float32)).requires_grad_()
    with pytest.raises(NotImplementedError, match=str(ops.HFIT_SINGLE_MAX)):       # (host tensors: not even a copy is made)
        L.find_homography_nonhomogeneous_QR(a, b, w)
    assert "forward only" in L.find_homography_IRLSq_QR.__doc__.lower()
    assert "forward only" in L.find_homography_cvransac.__doc__.lower() and "forward only" in L.find_homography_TRS.__doc__.lower()
