"""CPU checks of the batched homography fit's boundary (no GPU): `woft_hfit_batched` is exported, declared and rejects bad
arguments before any launch; the shim exports the projection-error helpers of least_squares_H.py:400-505 and a training
config in the reference's form (tests/configs/training_forms.py) imports; the helpers, which are plain torch / numpy ops on
the caller's device, reproduce on host tensors what the reference returned for the fixture tests/golden/reproj_errors.npz
(tools/gen_golden_reproj.py).

Tolerance of the fixture comparison: the one the existing test of torch_proj_errors uses (tests/test_homography_gpu.py:
rtol 1e-5, atol 1e-4) for the float32 torch helpers; the fixture's points lie in [0, 16]^2 and its homographies are within
5 % of the identity with at most half a pixel of translation (condition number below 2), where a float32 evaluation of
inv(E) G p, the division by z and the difference to the point (about a dozen roundings of 2^-24 relative to values of size
<= 20, amplified by the condition number of the inverted matrix) stays below 3e-5 px whatever the order of the operations,
so two float32 evaluations differ by less than 6e-5 px.  The float64 numpy helper is held to rtol 1e-9 (a 3x3 inverse and
two 3-term dot products in float64 on matrices of condition number below 2)."""
import ctypes
import re
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HELPERS = ("torch_reproj_errors", "torch_proj_diff_errors", "reproj_errors", "torch_H_proj", "torch_e2p", "torch_p2e")
RTOL, ATOL = 1e-5, 1e-4


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_batched_fit_exported_and_declared(lib):
    from woft_amd import _lib, ops
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    assert "woft_hfit_batched" in declared and "woft_hfit_batched" in _lib.EXPORTS
    raw = ctypes.CDLL(str(ROOT / "woft_amd" / "lib" / "libwoft_hip.so"))
    assert hasattr(raw, "woft_hfit_batched")
    m = re.search(r"#define\s+WOFT_HFIT_BATCH_MAX\s+(\d+)", header)
    assert m and int(m.group(1)) == ops.HFIT_BATCH_MAX            # (the documented bound and the host's chunk size agree)
    m = re.search(r"#define\s+WOFT_HFIT_SINGLE_MAX\s+(\d+)", header)
    assert m and int(m.group(1)) == ops.HFIT_SINGLE_MAX == 2048
    assert lib.woft_abi_version() == 400                          # (additions only: the version stays)


def test_batched_fit_rejects_bad_arguments_without_a_launch(lib):
    """NULL pa / pb / Hout / status, batch < 1 or above the bound, n_max < 1 and n_max > WOFT_HFIT_SINGLE_MAX -> WOFT_EINVAL.
    The non-NULL pointers are host addresses that no launch may see: there is no device here, the call must return first."""
    from woft_amd import ops
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok = dict(pa=p, pb=p, w=None, batch=2, n_max=4, counts=None, reweight=0, huber_k=1.0, n_irls=0, Hout=p, status=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.woft_hfit_batched(a["pa"], a["pb"], a["w"], a["batch"], a["n_max"], a["counts"], a["reweight"],
                                     a["huber_k"], a["n_irls"], a["Hout"], a["status"], None)
    for bad in (dict(pa=None), dict(pb=None), dict(Hout=None), dict(status=None), dict(batch=0), dict(batch=-3),
                dict(batch=ops.HFIT_BATCH_MAX + 1), dict(n_max=0), dict(n_max=-1), dict(n_max=2049),
                dict(reweight=3), dict(reweight=-1), dict(n_irls=-1)):
        assert call(**bad) == -1, bad
    assert lib.woft_hfit_batched(None, None, None, 1, 4, None, 0, 1.0, 0, None, None, None) == -1


def test_shim_exports_the_error_helpers():
    import pytracking.utils.least_squares_H as L
    import woft_amd.homography as Hm
    for name in HELPERS:
        assert callable(getattr(L, name)), name
        assert getattr(L, name) is getattr(Hm, name)
    for name in ("find_homography_nonhomogeneous_QR", "find_homography_IRLSq_QR", "torch_proj_errors"):
        assert callable(getattr(L, name)), name
    assert "forward only" in Hm.torch_reproj_errors.__doc__.lower()      # (no autograd through the HIP fit: documented)


def test_training_config_in_the_reference_form_imports():
    sys.dont_write_bytecode = True
    path = ROOT / "tests" / "configs" / "training_forms.py"
    m = types.ModuleType("training_config")
    m.__file__ = str(path)
    exec(compile(path.read_text(), str(path), "exec"), m.__dict__)
    conf = m.get_config()
    import woft_amd.homography as Hm
    assert conf.train.H_estimator is Hm.find_homography_nonhomogeneous_QR
    assert conf.train.loss_fn is Hm.torch_reproj_errors
    assert not re.search(r"^\s*(from|import)\s+woft_amd\b", path.read_text(), flags=re.M)


def test_error_helpers_reproduce_the_reference_fixture_on_host_tensors(golden_dir):
    import pytracking.utils.least_squares_H as L
    g = np.load(golden_dir / "reproj_errors.npz")
    G, E, P = (torch.from_numpy(g[k]) for k in ("GT_H", "est_H", "pts"))
    assert tuple(G.shape) == (4, 3, 3) and tuple(P.shape) == (4, 2, 16) and G.dtype == torch.float32
    got = {"torch_reproj_errors": L.torch_reproj_errors(G, E, P), "torch_proj_diff_errors": L.torch_proj_diff_errors(G, E, P),
           "torch_H_proj": L.torch_H_proj(G, P), "torch_e2p": L.torch_e2p(P),
           "torch_p2e": L.torch_p2e(torch.matmul(G, L.torch_e2p(P)))}
    for name, v in got.items():
        ref = g[name]
        assert tuple(v.shape) == ref.shape and v.dtype == torch.float32, name
        err = float(np.abs(v.numpy().astype(np.float64) - ref).max())
        print(f"[reproj fixture, host] {name}: max |diff| {err:.3e}")
        assert np.allclose(v.numpy(), ref, rtol=RTOL, atol=ATOL), (name, err)
    assert np.array_equal(got["torch_e2p"].numpy()[:, 2], np.ones((4, 16), np.float32))
    assert float(g["torch_reproj_errors"].min()) > 10 * ATOL          # (the errors are not lost in the tolerance)
    g64, e64, p64 = (g[k].astype(np.float64) for k in ("GT_H", "est_H", "pts"))
    for b in range(4):
        m = L.reproj_errors(g64[b], e64[b], p64[b])
        assert isinstance(m, float) and np.isclose(m, g["reproj_errors_mean"][b], rtol=1e-9, atol=0)
        e = L.reproj_errors(g64[b], e64[b], p64[b], mean=False)
        assert e.shape == (16,) and np.allclose(e, g["reproj_errors_all"][b], rtol=1e-9, atol=0)
