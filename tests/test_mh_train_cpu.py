"""CPU checks of the mask-head training path: the new C ABI entry points' symbols and argument validation
(no GPU here), the parameter names against the synthetic checkpoint's keys, and the restatement the GPU tests compare with
(tests/mh_train_host.py) against itself in float64."""
import ctypes

import pytest
import torch

import mh_train_host as host
from woft_amd import synth

NEW = ("woft_mh_train_conv", "woft_mh_wgrad_ws_bytes", "woft_mh_wgrad", "woft_mh_reduce_bwd")


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_new_symbols_exported_and_abi_version(lib):
    from woft_amd import _lib, ops
    header = (_lib.LIB_PATH.parent.parent.parent / "include" / "woft_hip.h").read_text()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert lib.woft_abi_version() == 400
    for macro, value in (("WOFT_MH_TRAIN_TILE", ops.MH_TRAIN_TILE), ("WOFT_MH_TRAIN_CHUNK", ops.MH_TRAIN_CHUNK),
                         ("WOFT_MH_REDUCE_CHUNK", ops.MH_REDUCE_CHUNK)):
        assert f"#define {macro} {value}\n" in header, macro


def test_new_entry_points_validate_without_gpu(lib):
    """NULL pointers and out-of-range sizes return -1 before any launch."""
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    conv = lib.woft_mh_train_conv
    assert conv(None, 64, None, 0, 64, 64, p, 32, p, None, 0, 2, 2, p, 32, None) == -1
    assert conv(p, 64, None, 0, 64, 64, None, 32, p, None, 0, 2, 2, p, 32, None) == -1
    assert conv(p, 64, None, 0, 64, 64, p, 32, p, None, 0, 2, 2, None, 32, None) == -1
    assert conv(p, 64, None, 0, 64, 64, p, 48, p, None, 0, 2, 2, p, 48, None) == -1            # cout not a multiple of 32
    assert conv(p, 64, None, 0, 64, 64, p, 160, p, None, 0, 2, 2, p, 160, None) == -1          # cout above 128
    assert conv(p, 48, None, 0, 48, 48, p, 32, p, None, 0, 2, 2, p, 32, None) == -1            # cin not a multiple of 32
    assert conv(p, 544, None, 0, 544, 544, p, 32, p, None, 0, 2, 2, p, 32, None) == -1         # cin above 512
    assert conv(p, 64, None, 0, 32, 64, p, 32, p, None, 0, 2, 2, p, 32, None) == -1            # a split without a second source
    assert conv(p, 64, p, 32, 64, 64, p, 32, p, None, 0, 2, 2, p, 32, None) == -1              # a second source without a split
    assert conv(p, 32, p, 16, 32, 64, p, 32, p, None, 0, 2, 2, p, 32, None) == -1              # second source's stride too small
    assert conv(p, 32, None, 0, 64, 64, p, 32, p, None, 0, 2, 2, p, 32, None) == -1            # first source's stride too small
    assert conv(p, 64, None, 0, 64, 64, p, 32, p, p, 32, 2, 2, p, 32, None) == -1              # bias and gate
    assert conv(p, 64, None, 0, 64, 64, p, 32, None, p, 16, 2, 2, p, 32, None) == -1           # gate stride too small
    assert conv(p, 64, None, 0, 64, 64, p, 32, p, None, 0, 2, 2, p, 16, None) == -1            # output stride too small
    assert conv(p, 64, None, 0, 64, 64, p, 32, p, None, 0, 0, 2, p, 32, None) == -1
    assert conv(p, 64, None, 0, 64, 64, p, 32, p, None, 0, 2, -1, p, 32, None) == -1
    wgrad = lib.woft_mh_wgrad
    assert wgrad(None, 32, 32, p, 64, None, 0, 64, 64, 2, 2, p, p, p, None) == -1
    assert wgrad(p, 32, 32, p, 64, None, 0, 64, 64, 2, 2, None, p, p, None) == -1
    assert wgrad(p, 32, 32, p, 64, None, 0, 64, 64, 2, 2, p, None, p, None) == -1
    assert wgrad(p, 32, 32, p, 64, None, 0, 64, 64, 2, 2, p, p, None, None) == -1
    assert wgrad(p, 16, 32, p, 64, None, 0, 64, 64, 2, 2, p, p, p, None) == -1                 # gradient stride too small
    assert wgrad(p, 48, 48, p, 64, None, 0, 64, 64, 2, 2, p, p, p, None) == -1
    assert wgrad(p, 32, 32, p, 64, None, 0, 64, 64, 0, 2, p, p, p, None) == -1
    assert lib.woft_mh_wgrad_ws_bytes(0, 4, 64, 32) == -1 and lib.woft_mh_wgrad_ws_bytes(4, 4, 48, 32) == -1
    assert lib.woft_mh_wgrad_ws_bytes(4, 4, 64, 160) == -1
    # 17 rows of 33 pixels = 34 tiles = 3 chunks of 16 tiles
    assert lib.woft_mh_wgrad_ws_bytes(17, 33, 64, 32) == 3 * (9 * 32 * 64 + 32) * 4
    # 1080p: 135 rows of 8 tiles = 68 chunks
    assert lib.woft_mh_wgrad_ws_bytes(135, 240, 512, 128) == 68 * (9 * 128 * 512 + 128) * 4
    red = lib.woft_mh_reduce_bwd
    assert red(None, 32, 32, p, p, 4, p, 32, p, p, p, None) == -1
    assert red(p, 32, 32, p, p, 0, p, 32, p, p, p, None) == -1
    assert red(p, 32, 48, p, p, 4, p, 48, p, p, p, None) == -1
    assert red(p, 16, 32, p, p, 4, p, 32, p, p, p, None) == -1
    assert red(p, 32, 32, p, p, 4, p, 16, p, p, p, None) == -1
    assert red(p, 32, 32, p, p, 4, p, 32, None, p, p, None) == -1


@pytest.mark.parametrize("structure", [[(64, 3)], [(128, 3), (128, 3)], [(32, 3), (64, 3), (96, 3)]])
def test_parameter_names_are_the_checkpoints(structure):
    from woft_amd import mh_train
    sd = synth.make_state_dict(seed=2, mask_head_structure=structure)
    keys = [k for k in sd if k.startswith("mask_head.net.")]
    assert sorted(keys) == sorted(mh_train.names(len(structure)))
    assert list(mh_train.names(1)) == ["mask_head.net.0.weight", "mask_head.net.0.bias", "mask_head.net.2.weight",
                                       "mask_head.net.2.bias"]
    shapes = [tuple(sd[f"mask_head.net.{2 * k}.weight"].shape) for k in range(len(structure) + 1)]
    assert mh_train.refusal(shapes) is None


def test_refusal_names_the_reason():
    from woft_amd import mh_train
    assert "kernel size 5" in mh_train.refusal([(128, 512, 5, 5), (1, 128, 1, 1)])
    assert "48 channels" in mh_train.refusal([(48, 512, 3, 3), (1, 48, 1, 1)])
    assert "160 channels" in mh_train.refusal([(128, 512, 3, 3), (160, 128, 3, 3), (1, 160, 1, 1)])


@pytest.mark.parametrize("do_sigmoid", [False, True])
def test_restatement_float32_agrees_with_float64(do_sigmoid):
    """Values and gradients of the restatement on a 3 x 5 map, float32 against float64: the yardstick of the GPU tests is sane
    (a float32 restatement that disagreed with float64 by more than rounding would make their bound meaningless)."""
    g = torch.Generator().manual_seed(4)
    hf, wf, cin = 3, 5, 64
    x = torch.randn(1, cin, hf, wf, generator=g)
    params = host.random_params(g, cin, (32, 64))
    mask = torch.randn(hf * wf, 576, generator=g) * 2
    pts = torch.stack([torch.randint(0, 8 * wf, (30,), generator=g), torch.randint(0, 8 * hf, (30,), generator=g)], 1).float()
    pts[:4] = torch.tensor([[0, 0], [8 * wf - 1, 0], [0, 8 * hf - 1], [8 * wf - 1, 8 * hf - 1]]).float()
    g_out = torch.randn(30, generator=g)
    v64, g64 = host.autograd(x, params, mask, pts, hf, wf, (0, 0), g_out, do_sigmoid, torch.float64)
    v32, g32 = host.autograd(x, params, mask, pts, hf, wf, (0, 0), g_out, do_sigmoid, torch.float32)
    assert host.rel_err(v32, v64) <= 1e-5
    for a, b in zip(g32, g64):
        assert a.shape == b.shape and host.rel_err(a, b) <= 1e-5
