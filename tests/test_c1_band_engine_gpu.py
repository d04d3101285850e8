"""convc1 on the correlation band in the engine (woft_conv1x1_band in place of conv2(convc1, convf1); engine.FUSE_C1): whole
flows and tracker runs with the fused form on and off are bit-identical -- every precision with a band, restricted last iterations
and the deferred weight head, eagerly and as a replayed hipGraph, a run whose blocks really miss -- and a launch trace shows the
three launches of an unrestricted iteration and the untouched final lookup.  (The set-ups of test_lookup_band_engine_gpu.py.)"""
from pathlib import Path

import numpy as np
import pytest
import torch

from woft_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _provider(sd, iters, precision, fuse_c1, graph=False):
    from woft_amd.config import Config
    from woft_amd.flow_provider import RAFTWrapper
    c = Config()
    c.of_class = RAFTWrapper
    c.raft_type = "weighted"
    c.class_params = Config()
    c.class_params.small = False
    c.class_params.mixed_precision = False
    c.class_params.alternate_corr = False
    c.class_params.weight_head_structure = [(128, 3)] * 3
    c.model, c.iters, c.padding_mode, c.precision, c.corr_band, c.fuse_c1 = sd, iters, "nopad", precision, True, fuse_c1
    c.graph = graph
    return c.of_class(c)


def _pair(h, w, seq_id):
    a = synth.make_template(h, w, seq_id=seq_id)
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (a, synth.make_frame(a, 2))]


def _names(fn):
    """The entry points fn() calls, and the recorded calls (launch_trace.LibProxy)."""
    from launch_trace import LibProxy
    proxy = LibProxy(_lib.load())
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(_lib, "_lib", proxy)
        fn()
        torch.cuda.synchronize()
    return [name for name, _, _ in proxy.calls], proxy.calls


def test_the_switch_is_on_by_default():
    assert engine.FUSE_C1 and _provider(synth.make_state_dict(seed=3), 2, "bf16x3", None).engine.fuse_c1 is True


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp16"])
@pytest.mark.parametrize("h,w", [(136, 200), (128, 160)])
def test_whole_flows_are_unchanged(h, w, precision):
    """12 iterations: flow, weights and correspondences with the fused form equal those of the three launches."""
    sd = synth.make_state_dict(seed=3)
    a, b = _pair(h, w, 2)
    outs = {}
    for fuse in (False, True):
        prov = _provider(sd, 12, precision, fuse)
        assert prov.engine.fuse_c1 is fuse
        names, _ = _names(lambda: prov.compute_flow(a, b, mode="flow", do_sigmoid=True))
        assert ("woft_conv1x1_band" in names) == fuse and prov.engine.plan(h, w).band_valid
        flow, wts = prov.compute_flow(a, b, mode="flow", do_sigmoid=True)
        _, dst, wtc = prov.compute_flow(a, b, mode="TC", do_sigmoid=True)
        outs[fuse] = [t.clone() for t in (flow, wts, dst, wtc)]
    for x, y in zip(outs[False], outs[True]):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


@pytest.mark.parametrize("graph", [False, True])
def test_flow_region_and_deferred_weights_are_unchanged(graph):
    """12 iterations with restricted last iterations (they keep their three launches), the weight head on a region and deferred
    weights (the final lookup with `need`), eagerly and as a replayed hipGraph."""
    from pytracking.utils.config import load_config
    H, W = 256, 320
    sd = synth.make_state_dict(seed=11)
    template = synth.make_template(H, W, seq_id=4)
    frame = synth.make_frame(template, 2)
    mask = np.zeros((H, W), bool)
    mask[8:40, 264:296] = True
    sel = torch.from_numpy(mask.reshape(-1)).cuda()
    ys, xs = np.nonzero(mask)
    pick = np.random.default_rng(0).choice(ys.size, 300, replace=False)
    pts = torch.from_numpy(np.stack([xs[pick], ys[pick]], 1).astype(np.float32)).cuda()
    count = torch.tensor([300], dtype=torch.int32, device="cuda")
    outs = {}
    for fuse in (False, True):
        conf = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
        conf.flow_config.model, conf.flow_config.iters, conf.flow_config.precision = sd, 12, "bf16x3"
        conf.flow_config.graph, conf.flow_config.corr_band, conf.flow_config.fuse_c1 = graph, True, fuse
        fl = conf.tracker_class(conf).flower
        assert fl.engine.fuse_c1 is fuse
        fl.pin_source(template)
        fl.pin_weight_region(mask)
        fl.pin_flow_region(mask)
        fl.defer_min_ratio = 0
        plan = fl.engine.plan(H, W)
        for _ in range(3 if graph else 1):                    # (graph: the third call replays the capture)
            flow, w = fl.compute_flow(template, frame, mode="flow", do_sigmoid=True, weight_region=True, flow_region=True)
            assert plan.flow_region is not None
            _, dst, none = fl.compute_flow(template, frame, mode="TC", do_sigmoid=True, weight_region=True, flow_region=True,
                                           defer_weights=300, borrow=True)
            assert fl.weights_deferred and none is None and plan.band_valid
            wp = fl.finish_weights(pts, count, 300, out=torch.zeros(300, device="cuda")).clone()
            res = [flow.reshape(2, -1)[:, sel].clone(), w.reshape(1, -1)[:, sel].clone(), dst[:, sel].clone(), wp]
        if graph:
            assert any(g is not None for g in plan._graphs.values()), "nothing was replayed"
        outs[fuse] = res
    for x, y in zip(outs[False], outs[True]):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


def test_tracker_results_when_blocks_really_miss():
    """Five frames at 256 x 320 with a flow head that drifts -0.65 cells per iteration along x (test_lookup_band_engine_gpu's
    second run): the last lookups of every frame leave the band, so the fused launch mixes sampled blocks with rows the
    fallback wrote.  Tracks and metas equal those of the three launches; the miss counter rises on every frame."""
    from pytracking.utils.config import load_config
    H, W = 256, 320
    sd = dict(synth.make_state_dict(seed=5))
    sd["update_block.flow_head.conv2.bias"] = sd["update_block.flow_head.conv2.bias"] + torch.tensor([-0.65, 0.0])
    template = synth.make_template(H, W, seq_id=6)
    frames = [synth.make_frame(template, t) for t in range(1, 6)]
    frames[3] = np.ascontiguousarray(np.roll(frames[3], 48, axis=1))
    mask = np.zeros((H, W), np.uint8)
    mask[60:150, 180:300] = 255
    outs, misses = {}, {}
    for fuse in (False, True):
        conf = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
        conf.flow_config.model, conf.flow_config.iters, conf.flow_config.precision = sd, 6, "bf16x3"
        conf.flow_config.corr_band, conf.flow_config.fuse_c1 = "auto", fuse
        trk = conf.tracker_class(conf)
        trk.init(template, mask)
        plan = trk.flower.engine.plan(H, W)
        res, seen = [], []
        for f in frames:
            Hm, meta = trk.track(f)
            res.append((Hm, dict(vars(meta))))
            seen.append(plan.band_miss_blocks)
        assert plan._band is not None
        outs[fuse], misses[fuse] = res, seen
    print(f"C1 BAND missed blocks after each frame: {misses[True]}")
    assert min(misses[True]) > 0 and misses[True] == misses[False]
    for (ha, ma), (hb, mb) in zip(outs[False], outs[True]):
        assert np.array_equal(ha, hb) and ma.keys() == mb.keys()
        for key in ma:
            a, b = ma[key], mb[key]
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, key


def test_launches_of_a_fused_flow():
    """With the fused form on, every unrestricted iteration calls woft_corr_lookup_band with the samples deferred, then
    woft_corr_lookup_otf on its miss flags, then woft_conv1x1_band on the same band parameters; no woft_conv2d_pair carries
    convc1 (324 -> 256 columns), and the final lookup, which feeds the weight head, writes its samples."""
    n = 6
    sd = synth.make_state_dict(seed=3)
    a, b = _pair(128, 160, 2)
    prov = _provider(sd, n, "bf16x3", True)
    names, calls = _names(lambda: prov.compute_flow(a, b, mode="flow"))
    band = [k for k, name in enumerate(names) if name == "woft_corr_lookup_band"]
    assert len(band) == n + 1 and names.count("woft_conv1x1_band") == n
    for j, k in enumerate(band):
        bp = calls[k][1][0]
        nxt, fb = calls[k + 1][0], calls[k + 1][1][0]
        assert nxt == "woft_corr_lookup_otf" and fb["need"] == bp["miss"] and fb["fh_part"] == 0
        if j < n:
            assert bp["defer_samples"] == 1 and names[k + 2] == "woft_conv1x1_band"
            c1, f1, bq = calls[k + 2][1][:3]
            assert (c1["cin_pad"], c1["cout_pad"], c1["in0"]) == (352, 256, bp["out"]) and f1["flat"] == 1
            assert bq["band"] == bp["band"] and bq["coords"] == bp["coords"] and bq["defer_samples"] == 0
        else:
            assert bp["defer_samples"] == 0 and names[k + 2] != "woft_conv1x1_band"
    for name, args, _ in calls:
        if name == "woft_conv2d_pair":
            assert 352 not in (args[0]["cin_pad"], args[1]["cin_pad"])
    # the switch off, a short flow (no band) and a warm start launch what they always did
    off = _provider(sd, n, "bf16x3", False)
    names_off, calls_off = _names(lambda: off.compute_flow(a, b, mode="flow"))
    assert "woft_conv1x1_band" not in names_off and names_off.count("woft_corr_lookup_band") == n + 1
    assert all(c[1][0]["defer_samples"] == 0 for c in calls_off if c[0] == "woft_corr_lookup_band")
    assert sum(1 for c in calls_off if c[0] == "woft_conv2d_pair" and c[1][0]["cin_pad"] == 352) == n
    short = _provider(sd, 3, "bf16x3", True)
    short.engine.corr_band = "auto"
    names_short, _ = _names(lambda: short.compute_flow(a, b, mode="flow"))
    assert "woft_conv1x1_band" not in names_short and "woft_corr_lookup_band" not in names_short
    names_warm, _ = _names(lambda: prov.compute_flow(a, b, mode="flow", flow_init=torch.zeros(2, 16, 20)))
    assert "woft_conv1x1_band" not in names_warm and "woft_corr_lookup_band" not in names_warm
