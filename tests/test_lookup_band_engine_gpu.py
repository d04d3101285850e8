"""The correlation band in the engine: whole flows and tracker runs with corr_band on and off are bit-identical (flow, weights,
correspondences; every precision with a split-bf16 correlation; restricted last iterations and the deferred weight head
included), long flows contain the band launches and short ones none, and the device miss counter moves only when a frame's
motion leaves the band."""
from pathlib import Path

import numpy as np
import pytest
import torch

from woft_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BAND_CALLS = ("woft_corr_band_build", "woft_corr_lookup_band")


def _provider(sd, iters, precision, corr_band, graph=False):
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
    c.model, c.iters, c.padding_mode, c.precision, c.corr_band = sd, iters, "nopad", precision, corr_band
    c.graph = graph
    return c.of_class(c)


def _pair(h, w, seq_id):
    a = synth.make_template(h, w, seq_id=seq_id)
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (a, synth.make_frame(a, 2))]


@pytest.mark.parametrize("precision", ["bf16x3", "bf16", "fp16"])
@pytest.mark.parametrize("h,w", [(136, 200), (128, 160)])
def test_whole_flows_are_unchanged(h, w, precision):
    """12 iterations: flow, weights and correspondences with the band equal those without, and the band really ran."""
    sd = synth.make_state_dict(seed=3)
    a, b = _pair(h, w, 2)
    outs = {}
    for band in (False, True):
        prov = _provider(sd, 12, precision, band)
        assert prov.engine.corr_band is band
        flow, wts = prov.compute_flow(a, b, mode="flow", do_sigmoid=True)
        _, dst, wtc = prov.compute_flow(a, b, mode="TC", do_sigmoid=True)
        plan = prov.engine.plan(h, w)
        assert plan.band_valid == band and (plan._band is not None) == band
        outs[band] = [t.clone() for t in (flow, wts, dst, wtc)]
    for x, y in zip(outs[False], outs[True]):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


@pytest.mark.parametrize("graph", [False, True])
def test_flow_region_and_deferred_weights_are_unchanged(graph):
    """The set-up of test_flow_region_engine_gpu with 12 iterations: restricted last iterations (roi_* / smp_* lookups), the weight
    head on a region, deferred weights (the final lookup with `need`), eagerly and as a replayed hipGraph."""
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
    for band in (False, True):
        conf = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
        conf.flow_config.model, conf.flow_config.iters, conf.flow_config.precision = sd, 12, "bf16x3"
        conf.flow_config.graph, conf.flow_config.corr_band = graph, band
        fl = conf.tracker_class(conf).flower
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
            assert fl.weights_deferred and none is None and plan.band_valid == band
            wp = fl.finish_weights(pts, count, 300, out=torch.zeros(300, device="cuda")).clone()
            res = [flow.reshape(2, -1)[:, sel].clone(), w.reshape(1, -1)[:, sel].clone(), dst[:, sel].clone(), wp]
        if graph:
            assert any(g is not None for g in plan._graphs.values()), "nothing was replayed"
        outs[band] = res
    for x, y in zip(outs[False], outs[True]):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


@pytest.mark.parametrize("drift", [0.0, 0.65])
def test_tracker_results_and_the_miss_counter(drift):
    """Five frames at 256 x 320, the fourth shifted by 48 pixels: identical track() results with the band on ("auto", 6
    iterations + the weight head's lookup) and off, and the miss counter stays at 0 on every frame -- the synthetic weights do
    not follow image motion (measured: no block misses even on the shifted frame), so a motion large enough to force misses
    is a second run whose flow head carries a bias of -`drift` cells per iteration along x: -3.25 cells after five updates,
    beyond the band, so the last lookups of every frame miss; the tracks are identical again and the counter rises.  (The
    template mask sits at the right so that the object, carried 31 pixels to the left per frame, stays in the image.)"""
    from pytracking.utils.config import load_config
    H, W = 256, 320
    sd = dict(synth.make_state_dict(seed=5))
    if drift:
        sd["update_block.flow_head.conv2.bias"] = sd["update_block.flow_head.conv2.bias"] + torch.tensor([-drift, 0.0])
    template = synth.make_template(H, W, seq_id=6)
    frames = [synth.make_frame(template, t) for t in range(1, 6)]
    frames[3] = np.ascontiguousarray(np.roll(frames[3], 48, axis=1))
    mask = np.zeros((H, W), np.uint8)
    mask[60:150, 180:300] = 255
    outs, misses = {}, None
    for band in (False, "auto"):
        conf = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
        conf.flow_config.model, conf.flow_config.iters, conf.flow_config.precision = sd, 6, "bf16x3"
        conf.flow_config.corr_band = band
        trk = conf.tracker_class(conf)
        trk.init(template, mask)
        plan = trk.flower.engine.plan(H, W)
        res, seen = [], []
        for f in frames:
            Hm, meta = trk.track(f)
            res.append((Hm, dict(vars(meta))))
            seen.append(plan.band_miss_blocks)
        assert (plan._band is not None) == (band == "auto")
        outs[band] = res
        if band == "auto":
            misses = seen
    print(f"BAND missed blocks after each frame: {misses}")
    for (ha, ma), (hb, mb) in zip(outs[False], outs["auto"]):
        assert np.array_equal(ha, hb) and ma.keys() == mb.keys()
        for key in ma:
            a, b = ma[key], mb[key]
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, key
    assert misses == [0] * 5 if not drift else min(misses) > 0


def test_long_flows_contain_the_band_launches_and_short_ones_none(monkeypatch):
    """corr_band = "auto": a flow of BAND_MIN_LOOKUPS iterations builds the band once, after the target pyramid, and every
    lookup is a band lookup followed by the volume-free lookup on the miss flags; 3 iterations, a warm start and exact fp32
    launch what they always did."""
    from launch_trace import LibProxy
    assert engine.BAND_MIN_LOOKUPS >= 6
    sd = synth.make_state_dict(seed=3)
    a, b = _pair(128, 160, 2)

    def trace(iters, precision="bf16x3", **kw):
        prov = _provider(sd, iters, precision, "auto")
        proxy = LibProxy(_lib.load())
        with pytest.MonkeyPatch.context() as patch:
            patch.setattr(_lib, "_lib", proxy)
            prov.compute_flow(a, b, mode="flow", **kw)
            torch.cuda.synchronize()
        return [name for name, _, _ in proxy.calls], proxy.calls

    n = engine.BAND_MIN_LOOKUPS
    names, calls = trace(n)
    assert names.count("woft_corr_band_build") == 1 and names.count("woft_corr_lookup_band") == n + 1
    assert names.index("woft_feature_pyramid") < names.index("woft_corr_band_build") < names.index("woft_corr_lookup_band")
    for k, name in enumerate(names):
        if name == "woft_corr_lookup_band":
            nxt, args = calls[k + 1][0], calls[k + 1][1][0]
            assert nxt == "woft_corr_lookup_otf" and args["need"] == calls[k][1][0]["miss"] and args["fh_part"] == 0
        elif name == "woft_corr_lookup_otf":
            assert names[k - 1] == "woft_corr_lookup_band"
    for kw in (dict(iters=3), dict(iters=n, flow_init=torch.zeros(2, 16, 20)), dict(iters=n, precision="fp32")):
        names, _ = trace(**kw)
        assert not any(x in names for x in BAND_CALLS) and "woft_corr_lookup_otf" in names


def test_a_replayed_graph_leaves_the_band_state_of_its_flow():
    """hipGraph replay does not run flow(): after the replay of a warm-started flow (no band; it overwrites the target pyramid)
    the plan must not believe the band of the flow before it, and after the replay of a band flow it must again -- the
    weight-head lookups that follow a flow (finish_weights, weights_at) go by that flag.  Results equal the eager provider's."""
    sd = synth.make_state_dict(seed=3)
    h, w = 128, 160
    a, b = _pair(h, w, 2)
    c = torch.from_numpy(np.ascontiguousarray(synth.make_frame(synth.make_template(h, w, seq_id=2), 3))).cuda()
    zero = torch.zeros(2, h // 8, w // 8)
    ref = _provider(sd, 6, "bf16x3", False)
    want = [t.clone() for t in ref.compute_flow(a, b, mode="flow", do_sigmoid=True)]
    prov = _provider(sd, 6, "bf16x3", True, graph=True)
    plan = prov.engine.plan(h, w)
    for _ in range(3):
        got = [t.clone() for t in prov.compute_flow(a, b, mode="flow", do_sigmoid=True)]
        assert plan.band_valid
    for _ in range(3):
        prov.compute_flow(a, c, mode="flow", do_sigmoid=True, flow_init=zero)
        assert not plan.band_valid
    assert sum(g is not None for g in plan._graphs.values()) == 2, "both flows must have been replayed"
    again = [t.clone() for t in prov.compute_flow(a, b, mode="flow", do_sigmoid=True)]
    assert plan.band_valid
    for x, y, z in zip(want, got, again):
        assert torch.equal(x, y) and torch.equal(x, z)
