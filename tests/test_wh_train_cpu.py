"""CPU checks of the weight-head training path: the stage-wise backward formulas that the kernels of
csrc/wh_train.hip implement against torch autograd of the whole restatement (tests/wh_train_host.py), the restatement against
the oracle's weight head + convex upsampling, and the new C ABI entry points' symbols and argument validation (no GPU here)."""
import ctypes

import pytest
import torch

import wh_train_host as host
from oracle import raft_ref
from woft_amd import synth

NEW = ("woft_convex_weights_at_bwd", "woft_wh_reduce_bwd", "woft_wh_train_conv", "woft_wh_wgrad_ws_bytes", "woft_wh_wgrad")


def _case(seed, hf=5, wf=6, crop=(2, 2), n_pts=40, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    P = hf * wf
    h, w = 8 * hf - 2 * crop[0], 8 * wf - 2 * crop[1]
    pts = torch.stack([torch.randint(0, w, (n_pts,), generator=g), torch.randint(0, h, (n_pts,), generator=g)], 1).float()
    pts[:4] = torch.tensor([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]).float()        # corners
    pts[5] = pts[4]                                                                          # a duplicate
    index = torch.arange(P, dtype=torch.int32)
    x5 = torch.randn(P, 5, 9, 9, generator=g)
    mask = torch.randn(P, 576, generator=g) * 2
    params = host.random_params(g)
    g_out = torch.randn(n_pts, generator=g)
    c = lambda t: t.to(dtype)
    return c(x5), [c(p) for p in params], index, c(mask), pts, hf, wf, crop, c(g_out)


@pytest.mark.parametrize("do_sigmoid", [False, True])
def test_stagewise_backward_equals_autograd_fp64(do_sigmoid):
    """The formulas per stage, in float64, against float64 autograd of the whole restatement: 1e-10 of the largest entry."""
    x5, params, index, mask, pts, hf, wf, crop, g_out = _case(1)
    got = host.backward(x5, params, index, mask, pts, hf, wf, crop, g_out, do_sigmoid)
    _, want = host.autograd(x5, params, index, mask, pts, hf, wf, crop, g_out, do_sigmoid)
    for name, a, b in zip(("w0", "b0", "w2", "b2", "w4", "b4", "w6", "b6"), got, want):
        assert a.shape == b.shape, name
        assert host.rel_err(a, b) <= 1e-10, (name, host.rel_err(a, b))


def test_restatement_matches_oracle():
    """head + upsample_at of the restatement = oracle.raft_ref.weight_head + convex_upsample on a small random trace."""
    g = torch.Generator().manual_seed(3)
    hf, wf = 4, 5
    P = hf * wf
    sd = {k: v.double() for k, v in synth.make_state_dict(seed=5).items() if k.startswith("weight_head.")}
    lookup = torch.randn(1, 324, hf, wf, generator=g, dtype=torch.float64)
    vol0 = torch.randn(P, 1, hf, wf, generator=g, dtype=torch.float64)
    mask = torch.randn(1, 576, hf, wf, generator=g, dtype=torch.float64)
    low = raft_ref.weight_head(sd, lookup, vol0, 4, hf, wf)
    up = raft_ref.convex_upsample(low, mask)[0, 0] / 8            # (as raft_forward takes the weights: the 8 * ... / 8 pair)
    rows = lookup[0].permute(1, 2, 0).reshape(P, 324)
    wmean = vol0.reshape(P, -1).mean(dim=1)
    index = torch.arange(P, dtype=torch.int32)
    x5 = host.x5_from_rows(rows, wmean, index)
    params = [sd[f"weight_head.net.{i}.{s}"] for i in (0, 2, 4, 6) for s in ("weight", "bias")]
    ys, xs = torch.meshgrid(torch.arange(8 * hf), torch.arange(8 * wf), indexing="ij")
    pts = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).float()
    got = host.weights_at(x5, params, index, mask[0].permute(1, 2, 0).reshape(P, 576), pts, hf, wf, (0, 0))
    assert float((got - up.reshape(-1)).abs().max()) <= 1e-12 * max(1.0, float(up.abs().max()))
    assert float((host.head(x5, params)[3] - low.reshape(-1)).abs().max()) <= 1e-12 * max(1.0, float(low.abs().max()))


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_new_symbols_exported_and_abi_version(lib):
    from woft_amd import _lib
    header = (_lib.LIB_PATH.parent.parent.parent / "include" / "woft_hip.h").read_text()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert lib.woft_abi_version() == 400


def test_new_entry_points_validate_without_gpu(lib):
    """NULL pointers and out-of-range sizes return -1 before any launch."""
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    assert lib.woft_convex_weights_at_bwd(None, None, 4, p, p, p, 576, 2, 2, 0, 0, 0, None, 4, p, None) == -1
    assert lib.woft_convex_weights_at_bwd(p, None, 0, p, p, p, 576, 2, 2, 0, 0, 0, None, 4, p, None) == -1
    assert lib.woft_convex_weights_at_bwd(p, None, 4, p, p, p, 575, 2, 2, 0, 0, 0, None, 4, p, None) == -1
    assert lib.woft_convex_weights_at_bwd(p, None, 4, p, None, p, 576, 2, 2, 0, 0, 1, None, 4, p, None) == -1   # sigmoid needs wlow
    assert lib.woft_convex_weights_at_bwd(p, None, 4, p, p, p, 576, 2, 2, 0, 0, 0, p, 5, p, None) == -1         # more windows than cells
    assert lib.woft_convex_weights_at_bwd(p, None, 4, p, p, p, 576, 2, 2, 0, 0, 0, None, 3, p, None) == -1
    assert lib.woft_wh_reduce_bwd(None, p, p, None, 1, p, p, p, p, None) == -1
    assert lib.woft_wh_reduce_bwd(p, p, p, None, 0, p, p, p, p, None) == -1
    assert lib.woft_wh_reduce_bwd(p, p, p, None, 9 * 2048 + 1, p, p, p, p, None) == -1
    assert lib.woft_wh_train_conv(None, 128, p, p, None, 1, p, None) == -1
    assert lib.woft_wh_train_conv(p, 64, p, p, None, 1, p, None) == -1
    assert lib.woft_wh_train_conv(p, 128, p, p, p, 1, p, None) == -1                                             # bias and gate
    assert lib.woft_wh_train_conv(p, 128, p, p, None, 0, p, None) == -1
    assert lib.woft_wh_wgrad(None, p, 128, 128, 1, p, p, p, None) == -1
    assert lib.woft_wh_wgrad(p, p, 8, 9, 1, p, p, p, None) == -1
    assert lib.woft_wh_wgrad(p, p, 32, 32, 1, p, p, p, None) == -1
    assert lib.woft_wh_wgrad(p, p, 128, 128, 9 * 2048 + 1, p, p, p, None) == -1
    assert lib.woft_wh_wgrad_ws_bytes(0, 128) == -1 and lib.woft_wh_wgrad_ws_bytes(16, 64) == -1
    assert lib.woft_wh_wgrad_ws_bytes(17, 128) == 2 * (9 * 128 * 128 + 128) * 4
