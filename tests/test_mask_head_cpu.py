"""CPU checks of the MaskHead surface ('weighted_masked'): the C entry point and its argument checks,
the synthetic checkpoint's mask-head tensors against the reference's recorded key list, and every configuration error of the
provider and the tracker -- all raised before any device work."""
import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_warp_features_declared_and_exported(lib):
    from woft_amd import _lib
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    assert "woft_warp_features" in declared and "woft_warp_features" in _lib.EXPORTS
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(raw, "woft_warp_features")


def test_warp_features_rejects_bad_arguments(lib):
    """Every rejected form returns -1 before any launch (host buffers stand in for device ones: nothing is dereferenced)."""
    buf = (ctypes.c_float * 4096)()
    a = ctypes.addressof(buf)
    assert a % 16 == 0
    good = dict(f=a, h=8, w=9, c=128, cs=128, coords=a + 64, n=10, out=a + 128, ld=128)

    def call(**kw):
        d = dict(good, **kw)
        return lib.woft_warp_features(d["f"], d["h"], d["w"], d["c"], d["cs"], d["coords"], d["n"], d["out"], d["ld"], None)

    for bad in (dict(f=None), dict(coords=None), dict(out=None), dict(c=0), dict(c=-4), dict(c=126), dict(cs=124),
                dict(ld=124), dict(cs=130, c=128), dict(ld=130), dict(h=1), dict(w=1), dict(h=0), dict(n=-1),
                dict(f=a + 4), dict(out=a + 8)):
        assert call(**bad) == -1, bad
    assert call(n=0) == 0                       # nothing to do: no launch


def test_synth_mask_head_matches_the_reference_key_list():
    from woft_amd import synth
    g = np.load(GOLD / "mask_head_128x160_it4.npz")
    keys = json.loads(str(g["mask_head_keys"]))
    for name in ("full", "small"):
        st = json.loads(str(g[f"{name}_structure"]))
        sd = synth.make_state_dict(seed=int(g[f"{name}_seed"]), small=bool(int(g[f"{name}_small"])), mask_head_structure=st)
        mine = {k: list(v.shape) for k, v in sd.items() if k.startswith("mask_head.")}
        assert mine == keys[name], name


def test_synth_default_key_set_unchanged():
    from woft_amd import synth
    pinned = json.loads((GOLD / "state_dict_keys.json").read_text())
    sd = synth.make_state_dict(seed=7)
    assert {k: list(v.shape) for k, v in sd.items()} == pinned["weighted_full"]
    assert not any(k.startswith("mask_head.") for k in sd)
    with_head = synth.make_state_dict(seed=7, mask_head_structure=[(128, 3)])
    for k, v in sd.items():                     # the mask head is drawn last: every other tensor is the same
        assert np.array_equal(v.numpy(), with_head[k].numpy()), k


class _EngineReached(Exception):
    pass


def _flow_config(raft_type, mask_estimation=None, structure=None, sd_structure=None, small=False):
    from woft_amd import synth
    from woft_amd.config import Config
    from woft_amd.flow_provider import RAFTWrapper
    c = Config()
    c.of_class = RAFTWrapper
    c.raft_type = raft_type
    c.class_params = Config()
    c.class_params.small = small
    c.class_params.weight_head_structure = [(128, 3)] * 3
    if mask_estimation is not None:
        c.class_params.mask_estimation = mask_estimation
    if structure is not None:
        c.class_params.mask_head_structure = structure
    c.model = synth.make_state_dict(seed=3, small=small, weighted=raft_type != "orig", mask_head_structure=sd_structure)
    c.iters = 2
    c.padding_mode = "nopad"
    c.precision = "fp32"
    return c


@pytest.fixture
def engine_stub(monkeypatch):
    """Replaces the engine: reaching it means the configuration was accepted (no device is touched either way)."""
    from woft_amd import flow_provider
    seen = {}

    def stub(state_dict, **kw):
        seen.update(kw)
        raise _EngineReached()
    monkeypatch.setattr(flow_provider, "RaftEngine", stub)
    return seen


@pytest.mark.parametrize("small", [False, True])
def test_accepted_configurations_reach_the_engine(engine_stub, small):
    st = [(64, 5), 32]
    fc = _flow_config("weighted_masked", True, st, st, small=small)
    with pytest.raises(_EngineReached):
        fc.of_class(fc)
    assert engine_stub["mask_head"] is True and engine_stub["weighted"] is True
    # 'orig' ignores mask_estimation, as the reference does (plain RAFT has no head)
    fc = _flow_config("orig", True, st, None, small=small)
    with pytest.raises(_EngineReached):
        fc.of_class(fc)
    assert engine_stub["mask_head"] is False and engine_stub["weighted"] is False


@pytest.mark.parametrize("case,match", [
    (dict(raft_type="weighted_masked", mask_estimation=None, structure=[(128, 3)], sd_structure=[(128, 3)]), "mask_estimation"),
    (dict(raft_type="weighted_masked", mask_estimation=False, structure=[(128, 3)], sd_structure=[(128, 3)]), "mask_estimation"),
    (dict(raft_type="weighted", mask_estimation=True, structure=[(128, 3)], sd_structure=[(128, 3)]), "weighted_masked"),
    (dict(raft_type="weighted_masked", mask_estimation=True, structure=None, sd_structure=[(128, 3)]), "mask_head_structure"),
    (dict(raft_type="weighted_masked", mask_estimation=True, structure=[(128, 3)], sd_structure=[(64, 3)]), "checkpoint"),
    (dict(raft_type="weighted_masked", mask_estimation=True, structure=[(128, 3)], sd_structure=[(128, 5)]), "checkpoint"),
    (dict(raft_type="weighted_masked", mask_estimation=True, structure=[(128, 3)], sd_structure=[(128, 3), 32]), "checkpoint"),
    (dict(raft_type="weighted_masked", mask_estimation=True, structure=[(128, 3)], sd_structure=None), "checkpoint"),
    (dict(raft_type="weighted_masked", mask_estimation=True, structure=[(128, 4)], sd_structure=[(128, 3)]), "odd kernel"),
    (dict(raft_type="masked", mask_estimation=True, structure=[(128, 3)], sd_structure=[(128, 3)]), "Unknown RAFT type"),
])
def test_configuration_errors_before_device_work(engine_stub, case, match):
    fc = _flow_config(**case)
    with pytest.raises(ValueError, match=match):
        fc.of_class(fc)
    assert not engine_stub


def test_tracker_refuses_a_masked_flow_config():
    from woft_amd.config import Config
    from woft_amd.tracker import YAOFTrackerSingleControl
    c = Config()
    c.flow_config = Config()
    c.flow_config.raft_type = "weighted_masked"

    def never(cfg):
        raise AssertionError("the flow provider must not be built")
    c.flow_config.of_class = never
    with pytest.raises(ValueError, match="weighted_masked"):
        YAOFTrackerSingleControl(c)
