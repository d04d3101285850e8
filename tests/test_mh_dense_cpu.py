"""CPU checks of the dense visibility map's training path: the dense restatement the GPU tests compare
with (tests/mh_dense_host.py) against the point-wise one already pinned (tests/wh_train_host.py), and the argument validation of
woft_convex_upsample_bwd (no GPU here)."""
import ctypes

import pytest
import torch

import mh_dense_host as host
import wh_train_host

NEW = ("woft_convex_upsample_bwd_ws_bytes", "woft_convex_upsample_bwd")


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("do_sigmoid", [False, True])
def test_dense_restatement_is_the_pointwise_one(do_sigmoid):
    """float64: upsample_dense = upsample_at at every pixel of a cropped (3, 5)-cell map, to 1e-12."""
    g = torch.Generator().manual_seed(11)
    hf, wf, crop, h, w = 3, 5, (2, 3), 19, 34
    low = torch.randn(hf * wf, generator=g, dtype=torch.float64)
    mask = torch.randn(hf * wf, 576, generator=g, dtype=torch.float64) * 2
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    pts = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).double()
    dense = host.upsample_dense(low, mask, hf, wf, crop, h, w, do_sigmoid)
    at = wh_train_host.upsample_at(low, mask, pts, hf, wf, crop, do_sigmoid).reshape(h, w)
    assert dense.shape == (h, w) and float((dense - at).abs().max()) <= 1e-12


def test_dense_gradient_is_the_pointwise_adjoint():
    """float64: autograd of upsample_dense with respect to the logits = wh_train_host.upsample_at_bwd over every pixel."""
    g = torch.Generator().manual_seed(12)
    hf, wf, crop, h, w = 3, 5, (2, 3), 19, 34
    low = torch.randn(hf * wf, generator=g, dtype=torch.float64)
    mask = torch.randn(hf * wf + 2, 640, generator=g, dtype=torch.float64) * 2
    g_up = torch.randn(h * w, generator=g, dtype=torch.float64)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    pts = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).double()
    for do_sigmoid in (False, True):
        got = host.low_grad(low, mask, hf, wf, crop, h, w, g_up, do_sigmoid)
        want = wh_train_host.upsample_at_bwd(g_up, low, mask, pts, hf, wf, crop, do_sigmoid)
        assert float((got - want).abs().max()) <= 1e-12


def test_symbols_exported_and_workspace_size(lib):
    from woft_amd import _lib
    header = (_lib.LIB_PATH.parent.parent.parent / "include" / "woft_hip.h").read_text()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert lib.woft_abi_version() == 400
    assert lib.woft_convex_upsample_bwd_ws_bytes(5, 7) == 9 * 35 * 4
    assert lib.woft_convex_upsample_bwd_ws_bytes(135, 240) == 9 * 32400 * 4          # 1080p
    assert lib.woft_convex_upsample_bwd_ws_bytes(0, 7) == -1 and lib.woft_convex_upsample_bwd_ws_bytes(5, -1) == -1


def test_entry_point_validates_without_gpu(lib):
    """NULL pointers, a short mask row, an empty map, a crop window that leaves the padded map and a sigmoid without its logits
    return -1 before any launch."""
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    bwd = lib.woft_convex_upsample_bwd
    #          g_up  mask  ld   wlow hf wf top left h   w  sig ws g_wlow stream
    assert bwd(None, p, 576, p, 2, 2, 0, 0, 16, 16, 0, p, p, None) == -1
    assert bwd(p, None, 576, p, 2, 2, 0, 0, 16, 16, 0, p, p, None) == -1
    assert bwd(p, p, 576, p, 2, 2, 0, 0, 16, 16, 0, p, None, None) == -1
    assert bwd(p, p, 576, p, 2, 2, 0, 0, 16, 16, 0, None, p, None) == -1              # no workspace
    assert bwd(p, p, 575, p, 2, 2, 0, 0, 16, 16, 0, p, p, None) == -1
    assert bwd(p, p, 576, p, 0, 2, 0, 0, 16, 16, 0, p, p, None) == -1
    assert bwd(p, p, 576, p, 2, 0, 0, 0, 16, 16, 0, p, p, None) == -1
    assert bwd(p, p, 576, p, 2, 2, 0, 0, 0, 16, 0, p, p, None) == -1
    assert bwd(p, p, 576, p, 2, 2, 0, 0, 16, -1, 0, p, p, None) == -1
    assert bwd(p, p, 576, p, 2, 2, 1, 0, 16, 16, 0, p, p, None) == -1                 # crop_top + h > 8 hf
    assert bwd(p, p, 576, p, 2, 2, 0, 3, 16, 14, 0, p, p, None) == -1                 # crop_left + w > 8 wf
    assert bwd(p, p, 576, p, 2, 2, -1, 0, 16, 16, 0, p, p, None) == -1
    assert bwd(p, p, 576, p, 2, 2, 0, -1, 16, 16, 0, p, p, None) == -1
    assert bwd(p, p, 576, None, 2, 2, 0, 0, 16, 16, 1, p, p, None) == -1              # the sigmoid needs wlow
