"""The refinement loop restricted to what a rectangle of the flow depends on (engine._Plan.set_flow_region, flow_provider.
pin_flow_region, the tracker's global stage): inside the declared mask everything the caller reads is bit-identical to the
unrestricted run, everything is finite everywhere, eagerly and as a replayed hipGraph; the tracker's results do not change."""
from pathlib import Path

import numpy as np
import pytest
import torch

from woft_amd import synth

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
H, W, ITERS = 256, 320, 4                # 32 x 40 cells
MASK = (slice(8, 40), slice(264, 296))   # 4 x 4 cells at rows 1-4, columns 33-36: the regions clip at the top and right borders


@pytest.fixture(scope="module")
def scene():
    sd = synth.make_state_dict(seed=11)
    template = synth.make_template(H, W, seq_id=4)
    frame = synth.make_frame(template, 2)
    mask = np.zeros((H, W), bool)
    mask[MASK] = True
    return sd, template, frame, mask


def _provider(sd, precision, graph=False):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
    conf.flow_config.model, conf.flow_config.iters, conf.flow_config.precision = sd, ITERS, precision
    conf.flow_config.graph = graph
    return conf.tracker_class(conf).flower


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_flow_inside_the_mask_is_unchanged(scene, precision, graph):
    sd, template, frame, mask = scene
    fl = _provider(sd, precision, graph)
    assert fl.use_graph == graph
    fl.pin_source(template)
    fl.pin_weight_region(mask)
    fl.pin_flow_region(mask)
    fl.defer_min_ratio = 0
    sel = torch.from_numpy(mask.reshape(-1)).cuda()
    ys, xs = np.nonzero(mask)
    pick = np.random.default_rng(0).choice(ys.size, 300, replace=False)
    pts = torch.from_numpy(np.stack([xs[pick], ys[pick]], 1).astype(np.float32)).cuda()
    count = torch.tensor([300], dtype=torch.int32, device="cuda")
    plan = fl.engine.plan(H, W)

    def run(region, reps):
        out = None
        for _ in range(reps):                                 # (graph: the third call replays the capture)
            flow, w = fl.compute_flow(template, frame, mode="flow", do_sigmoid=True, weight_region=True, flow_region=region)
            restricted = plan.flow_region is not None
            _, dst, wtc = fl.compute_flow(template, frame, mode="TC", do_sigmoid=True, weight_region=True, flow_region=region)
            _, dst2, none = fl.compute_flow(template, frame, mode="TC", do_sigmoid=True, weight_region=True, flow_region=region,
                                            defer_weights=300, borrow=True)
            # (exact fp32 has no fused weight head, hence no weight region and nothing deferred: the weights come with the call)
            assert fl.weights_deferred == (precision == "bf16x3") and (none is None) == fl.weights_deferred
            if fl.weights_deferred:
                wp = fl.finish_weights(pts, count, 300, out=torch.zeros(300, device="cuda")).clone()
            else:
                wp = none[0, torch.from_numpy(ys[pick] * W + xs[pick]).cuda()].clone()
            out = (flow, w, dst, wtc, dst2.clone(), wp, restricted)
        torch.cuda.synchronize()
        return out

    reps = 3 if graph else 1
    ref = run(False, reps)
    got = run(True, reps)
    assert not ref[6]
    # (exact fp32 runs the flow head as two launches and every conv on the per-tap kernel: nothing to restrict, by design)
    assert got[6] == (precision == "bf16x3")
    if graph:
        assert any(g is not None for g in plan._graphs.values()), "nothing was replayed"
        if got[6]:
            assert any(k.flow_region is not None and g is not None for k, g in plan._graphs.items()), "the restricted flow was not replayed"
    for t in got[:6]:
        assert bool(torch.isfinite(t).all())
    assert torch.equal(got[0].reshape(2, -1)[:, sel], ref[0].reshape(2, -1)[:, sel])        # flow_up
    assert torch.equal(got[1].reshape(1, -1)[:, sel], ref[1].reshape(1, -1)[:, sel])        # weights (mask region)
    assert torch.equal(got[2][:, sel], ref[2][:, sel]) and torch.equal(got[3][:, sel], ref[3][:, sel])   # dst, weights (TC)
    assert torch.equal(got[4][:, sel], ref[4][:, sel]) and torch.equal(got[5], ref[5])      # deferred: dst, weights at drawn points
    if got[6]:
        assert not torch.equal(got[0], ref[0]), "the restricted run computed the whole map"
        rects = plan.flow_region["rects"]
        last = [rr for it, tag, rr in rects if it == ITERS - 1 and tag == "convm"][0][0]
        assert last[0] == 0 and last[1] + last[3] == plan.wf and last[2] < plan.hf and last[3] < plan.wf     # clipped at two borders
    # a direct call never gets the region
    fl.compute_flow(template, frame, mode="flow", do_sigmoid=True)
    assert plan.flow_region is None
    # ... nor does a call with a warm start, and a frame-filling mask restricts nothing
    fl.compute_flow(template, frame, mode="flow", do_sigmoid=True, flow_region=True, flow_init=torch.zeros(2, H // 8, W // 8))
    assert plan.flow_region is None
    fl.pin_flow_region(np.ones((H, W), bool))
    fl.compute_flow(template, frame, mode="flow", do_sigmoid=True, flow_region=True)
    assert plan.flow_region is None


@pytest.mark.parametrize("backend", ["device", "callables"])
def test_tracker_results_do_not_change(monkeypatch, backend):
    """A 12-frame clip with one overruled ("lost") frame: every track() result is the same with the region on and off."""
    from pytracking.utils.config import load_config
    monkeypatch.setenv("WOFT_FUSED", "1" if backend == "device" else "0")
    sd = synth.make_state_dict(seed=5)
    template = synth.make_template(H, W, seq_id=6)
    frames = [synth.make_frame(template, t) for t in range(1, 13)]
    mask = np.zeros((H, W), np.uint8)
    mask[60:150, 90:230] = 255
    outs = {}
    for region in (False, True):
        conf = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
        conf.flow_config.model, conf.flow_config.iters, conf.flow_config.precision = sd, 6, "bf16x3"
        conf.flow_config.flow_region = region
        trk = conf.tracker_class(conf)
        assert (trk._fused is not None) == (backend == "device") and trk.flower.flow_region_on == region
        trk.init(template, mask)
        inner, k = trk._global_stage, {"i": -1}

        def overruled(frame, prewarp_H, inner=inner, k=k):
            fit = inner(frame, prewarp_H)
            k["i"] += 1
            if k["i"] == 5:
                fit.success = False
            return fit
        trk._global_stage = overruled
        plan = trk.flower.engine.plan(H, W)
        res, used = [], []
        for f in frames:
            Hm, meta = trk.track(f)
            used.append(plan.flow_region is not None)
            d = dict(vars(meta))
            res.append((Hm, d))
        assert [r[1]["lost"] for r in res] == [t == 5 for t in range(12)]
        assert used == [region] * 12                      # (plan = the template's buffer set: the global stage of every frame)
        assert trk.flower.engine.plan(H, W, 1).flow_region is None       # the lost frame's local flow: never restricted
        outs[region] = res
    for (ha, ma), (hb, mb) in zip(outs[False], outs[True]):
        assert np.array_equal(ha, hb) and ma.keys() == mb.keys()
        for key in ma:
            a, b = ma[key], mb[key]
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, key
