"""Warm start on the GPU: the two kernels against torch / the numpy restatement / the reference's golden
outputs (tests/golden/warm_start_128x160_it4.npz, tools/gen_golden_warm.py), the engine and the operator with a flow_init
against the reference network run with the same flow_init, zero == missing flow_init bit for bit, the round trip through
flow_low(), and the tracker's `warm_start_local`."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import warm_host  # noqa: E402
from woft_amd import presets, synth  # noqa: E402

FI_CASES = ["small_16x20", "large_16x20", "odd_17x23", "one_valid_16x20"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir / "warm_start_128x160_it4.npz")


def _flow_config(sd, iters, raft_type="weighted", structure=None, small=False, precision="fp32", corr=None, graph=False):
    from woft_amd.config import Config
    from woft_amd.flow_provider import RAFTWrapper
    c = Config()
    c.of_class = RAFTWrapper
    c.raft_type = raft_type
    c.class_params = Config()
    c.class_params.small = small
    c.class_params.mixed_precision = False
    c.class_params.alternate_corr = False
    c.class_params.weight_head_structure = [(128, 3)] * 3
    if raft_type == "weighted_masked":
        c.class_params.mask_estimation = True
        c.class_params.mask_head_structure = structure
    c.model = sd
    c.iters = iters
    c.padding_mode = "nopad"
    c.precision = precision
    if corr:
        c.corr = corr
    if graph:
        c.graph = True
    return c


def _epe(a, b):
    d = torch.as_tensor(a).detach().cpu().float() - torch.as_tensor(b).detach().cpu().float()
    e = torch.sqrt((d ** 2).sum(dim=-3))
    return float(e.mean()), float(e.max())


def _sig_err(a, b):
    a, b = torch.as_tensor(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)), torch.as_tensor(np.asarray(b))
    return float((torch.sigmoid(a.float().reshape(-1)) - torch.sigmoid(b.float().reshape(-1))).abs().max())


def _field(hf, wf, seed, scale=2.0):
    return (np.random.RandomState(seed).randn(2, hf, wf) * scale).astype(np.float32)


# ---- woft_coords_init_flow ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hf,wf", [(16, 20), (17, 23)])
def test_coords_init_flow_exact(hf, wf):
    from woft_amd import ops
    P = hf * wf
    f = _field(hf, wf, hf + wf)
    c = torch.full((P, 2), 7.0, device="cuda")
    f4 = torch.full((P, 4), 7.0, device="cuda")
    cat = torch.full((P, 16), 7.0, device="cuda")
    ops.coords_init_flow(c, torch.from_numpy(f).cuda(), hf, wf, f4, cat[:, 14:], 16)
    torch.cuda.synchronize()
    t = torch.from_numpy(f)
    ys, xs = torch.meshgrid(torch.arange(hf).float(), torch.arange(wf).float(), indexing="ij")
    want_c = torch.stack([xs + t[0], ys + t[1]], -1).reshape(P, 2)
    want_f = torch.stack([t[0], t[1]], -1).reshape(P, 2)
    assert torch.equal(c.cpu(), want_c)
    assert torch.equal(f4[:, :2].cpu(), want_f) and float(f4[:, 2:].abs().max()) == 0.0      # flow_init itself, (fx, fy, 0, 0)
    assert torch.equal(cat[:, 14:].cpu(), want_f) and bool((cat[:, :14] == 7.0).all())
    hc, hfl = warm_host.coords_init_flow(f)
    assert np.array_equal(c.cpu().numpy(), hc) and np.array_equal(f4[:, :2].cpu().numpy(), hfl)


@pytest.mark.parametrize("hf,wf", [(16, 20), (17, 23)])
def test_coords_init_flow_of_zeros_is_coords_init(hf, wf):
    from woft_amd import ops
    P = hf * wf
    bufs = []
    for zero_init in (False, True):
        c, f4, cat = (torch.full((P, n), 3.0, device="cuda") for n in (2, 4, 16))
        if zero_init:
            ops.coords_init_flow(c, torch.zeros(2, hf, wf, device="cuda"), hf, wf, f4, cat[:, 14:], 16)
        else:
            ops.coords_init(c, hf, wf, f4, cat[:, 14:], 16)
        bufs.append((c, f4, cat))
    torch.cuda.synchronize()
    for a, b in zip(*bufs):        # (bytes: a -0.0 would not be a zero flow)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- woft_forward_interpolate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FI_CASES)
def test_forward_interpolate_bit_equal_to_the_reference(gold, name):
    from woft_amd import forward_interpolate
    flow = torch.from_numpy(gold[f"fi_{name}_flow"]).cuda()
    out = forward_interpolate(flow)
    again = forward_interpolate(flow[None])                # (1, 2, hf, wf) form; the same result a second time
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(flow.shape) and tuple(again.shape) == (1,) + tuple(flow.shape)
    assert np.array_equal(out.cpu().numpy(), gold[f"fi_{name}_out"])
    assert torch.equal(out, again[0])


def test_forward_interpolate_all_invalid_gives_zeros():
    from woft_amd import ops
    for f in (torch.full((2, 16, 20), 1e6), torch.full((2, 17, 23), float("nan")), -torch.ones(2, 1, 1)):
        out = torch.full_like(f, 5.0).cuda()
        ops.forward_interpolate(f.cuda(), out)
        torch.cuda.synchronize()
        assert float(out.abs().max()) == 0.0


def test_forward_interpolate_tie_takes_the_lowest_index():
    from woft_amd import ops
    f = np.full((2, 3, 3), 100.0, np.float32)
    f[:, 0, 1] = (-0.5, 1.0)                               # point 1 -> (0.5, 1.0)
    f[:, 2, 1] = (0.5, -1.0)                               # point 7 -> (1.5, 1.0): both 0.25 from cell (1, 1)
    out = ops.forward_interpolate(torch.from_numpy(f).cuda()).cpu().numpy()
    assert tuple(out[:, 1, 1]) == (-0.5, 1.0)
    assert np.array_equal(out, warm_host.forward_interpolate(f))


@pytest.mark.parametrize("hf,wf,scale", [(40, 50, 6.0), (33, 47, 30.0)])
def test_forward_interpolate_many_chunks_and_blocks(hf, wf, scale):
    """More points than one LDS chunk (512) and more cells than one workgroup (128), sizes that divide neither; quarter-pixel
    flows make exact distance ties common, so the tie rule is exercised across chunk boundaries.  Deterministic: twice the same."""
    from woft_amd import ops
    f = np.round(_field(hf, wf, hf * wf, scale) * 4) / 4
    f = f.astype(np.float32)
    t = torch.from_numpy(f).cuda()
    a, b = ops.forward_interpolate(t), ops.forward_interpolate(t)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), warm_host.forward_interpolate(f))


# ---- engine and operator against the reference run with the same flow_init ------------------------------------------------
def _golden_case(gold, name):
    small = bool(int(gold[f"{name}_small"]))
    st = json.loads(str(gold[f"{name}_structure"])) if f"{name}_structure" in gold.files else None
    kw = dict(mask_head_structure=st) if st else {}
    sd = synth.make_state_dict(seed=int(gold[f"{name}_seed"]), small=small, weighted=True, **kw)
    src = str(gold[f"{name}_images"])
    return sd, small, st, gold[f"{src}_img1"], gold[f"{src}_img2"]


@torch.no_grad()
@pytest.mark.parametrize("name", ["full", "small", "masked"])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_operator_with_flow_init_vs_golden(gold, name, precision):
    """The bounds of tests/test_mask_head_gpu.py::test_operator_vs_golden (same image size, same iteration count): EPE mean 1e-3,
    max 1e-2; sigmoid of the weights and of the mask within 1e-4; flow_low within the EPE bounds / 8."""
    sd, small, st, img1, img2 = _golden_case(gold, name)
    fc = _flow_config(sd, int(gold["iters"]), "weighted_masked" if st else "weighted", st, small=small, precision=precision)
    flower = fc.of_class(fc)
    init = gold[f"{name}_flow_init"]
    # (the three accepted forms: numpy (1, 2, h, w), host tensor, device tensor)
    init = {"full": init[None], "small": torch.from_numpy(init), "masked": torch.from_numpy(init).cuda()}[name]
    res = flower.compute_flow(img1, img2, mode="flow", do_sigmoid=False, flow_init=init)
    low = flower.flow_low()
    torch.cuda.synchronize()
    flow, w = res[0], res[1]
    mean, mx = _epe(flow, gold[f"{name}_flow_up"][0])
    print(f"{name} {precision}: flow_up EPE mean {mean:.3e} max {mx:.3e}")
    assert mean < 1e-3 and mx < 1e-2, (mean, mx)
    e = _sig_err(w, gold[f"{name}_w_up"])
    print(f"{name} {precision}: weights {e:.3e}")
    assert e < 1e-4, e
    if st:
        e = _sig_err(res[2], gold[f"{name}_mask_up"])
        print(f"{name} {precision}: mask {e:.3e}")
        assert e < 1e-4, e
    assert tuple(low.shape) == (2, 16, 20) and low.is_cuda and low.is_contiguous()
    mean, mx = _epe(low, gold[f"{name}_flow_low"][0])
    print(f"{name} {precision}: flow_low EPE mean {mean:.3e} max {mx:.3e}")
    assert mean < 1e-3 / 8 and mx < 1e-2 / 8, (mean, mx)
    assert torch.equal(flower.flow_low(copy=False), low)


# ---- zero / missing flow_init, shapes, iters ------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("corr", ["otf", "volume"])
@pytest.mark.parametrize("graph", [False, True])
def test_zero_flow_init_is_bit_identical_to_none(gold, corr, graph):
    sd, small, st, img1, img2 = _golden_case(gold, "full")
    fc = _flow_config(sd, 3, precision="bf16x3", corr=corr, graph=graph)
    flower = fc.of_class(fc)
    assert flower.corr == corr and flower.use_graph == graph
    zeros = torch.zeros(2, 16, 20)
    outs = {}
    for tag, kw in (("none", {}), ("zeros", dict(flow_init=zeros)), ("none_again", {})):
        for _ in range(3 if graph else 1):                 # (graph: eager, eager + capture, replay -- the third call is the replay)
            flow, w = flower.compute_flow(img1, img2, mode="flow", do_sigmoid=False, **kw)
        outs[tag] = (flow, w, flower.flow_low())
    torch.cuda.synchronize()
    if graph:
        plan = next(iter(flower.engine._plans.values()))
        assert sum(g is not None for g in plan._graphs.values()) == 2          # one graph per "has a flow_init"
    for tag in ("zeros", "none_again"):
        for a, b in zip(outs["none"], outs[tag]):
            assert torch.equal(a, b), tag
    assert float(outs["none"][0].abs().max()) > 0.5


@torch.no_grad()
def test_graph_replay_reads_the_new_flow_init(gold):
    """A captured graph with a flow_init reads the plan's buffer: a different flow_init at the replay gives that call's eager result."""
    sd, small, st, img1, img2 = _golden_case(gold, "full")
    eager = _flow_config(sd, 3, precision="bf16x3")
    eager = eager.of_class(eager)
    fc = _flow_config(sd, 3, precision="bf16x3", graph=True)
    flower = fc.of_class(fc)
    a, b = gold["full_flow_init"], gold["masked_flow_init"]
    for init in (a, a, b):
        got = flower.compute_flow(img1, img2, mode="flow", flow_init=init)[0]
    want = eager.compute_flow(img1, img2, mode="flow", flow_init=b)[0]
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@torch.no_grad()
def test_wrong_shape_raises_and_iters_overrides(gold):
    sd, small, st, img1, img2 = _golden_case(gold, "small")
    fc = _flow_config(sd, 4, small=True, precision="bf16x3")
    flower = fc.of_class(fc)
    with pytest.raises(RuntimeError):
        flower.flow_low()
    for bad in (np.zeros((2, 20, 16), np.float32), torch.zeros(2, 16, 21), np.zeros((2, 2, 16, 20), np.float32),
                torch.zeros(2, 128, 160), np.zeros((2, 16, 20), np.int32)):
        with pytest.raises(ValueError, match=r"\(2, 16, 20\)"):
            flower.compute_flow(img1, img2, mode="flow", flow_init=bad)
    with pytest.raises(ValueError):
        flower.compute_flow(img1, img2, mode="flow", iters=0)
    f2 = flower.compute_flow(img1, img2, mode="flow", iters=2)[0]
    f4 = flower.compute_flow(img1, img2, mode="flow")[0]
    fc2 = _flow_config(sd, 2, small=True, precision="bf16x3")
    want2 = fc2.of_class(fc2).compute_flow(img1, img2, mode="flow")[0]
    torch.cuda.synchronize()
    assert torch.equal(f2, want2) and not torch.equal(f2, f4)


# ---- round trip -------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("small", [False, True])
def test_round_trip_starts_where_the_first_flow_ended(gold, small):
    sd, _, _, img1, img2 = _golden_case(gold, "small" if small else "full")
    fc = _flow_config(sd, 4, small=small, precision="bf16x3")
    flower = fc.of_class(fc)
    flower.compute_flow(img1, img2, mode="flow")
    low1 = flower.flow_low()
    plan = next(iter(flower.engine._plans.values()))
    seen = {}

    def trace(p, it):
        seen[it] = (p.flow4.t[:, :2].clone(), p.xbuf.t[:, p.eng.spec.flow_off:p.eng.spec.flow_off + 2].clone(), p.coords.clone())
    orig = plan.flow
    plan.flow = lambda *a, **kw: orig(*a, trace=trace, **kw)
    flower.compute_flow(img1, img2, mode="flow", flow_init=low1)
    low2 = flower.flow_low()
    torch.cuda.synchronize()
    assert sorted(seen) == [-1, 0, 1, 2, 3]
    start = low1.reshape(2, -1).t()
    assert torch.equal(seen[-1][0], start) and torch.equal(seen[-1][1], start)      # the first iteration's flow input
    ys, xs = torch.meshgrid(torch.arange(16.0), torch.arange(20.0), indexing="ij")
    grid = torch.stack([xs, ys], -1).reshape(-1, 2).cuda()
    assert torch.equal(seen[-1][2], grid + start)
    assert torch.equal(seen[3][0], low2.reshape(2, -1).t())                         # flow_low() is the last update's flow
    assert bool(torch.isfinite(low2).all())
    mean, mx = _epe(low2, low1)
    print(f"small={small}: |second flow_low - first| mean {mean:.3e} max {mx:.3e}")


# ---- tracker ----------------------------------------------------------------------------------------------------------
def _corner_dist(Ha, Hb, mask):
    ys, xs = np.nonzero(mask)
    c = np.array([[xs.min(), ys.min(), 1], [xs.max(), ys.min(), 1], [xs.max(), ys.max(), 1], [xs.min(), ys.max(), 1.0]]).T
    pa, pb = np.linalg.inv(Ha) @ c, np.linalg.inv(Hb) @ c
    return float(np.abs(pa[:2] / pa[2] - pb[:2] / pb[2]).max())


def _tracker(cfg, sd, iters, spy):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / cfg)
    conf.flow_config.model = sd
    conf.flow_config.iters = iters
    trk = conf.tracker_class(conf)
    trk.flower.defer_min_ratio = 0          # (the deferred weight head whatever the region's size: 320 windows here)
    orig = trk.flower.compute_flow

    def compute_flow(src, dst, **kw):
        out = orig(src, dst, **kw)
        init = kw.get("flow_init")
        spy.append(dict(local=src is not trk.template_img, init=None if init is None else init.clone(), iters=kw.get("iters"),
                        low=trk.flower.flow_low(), deferred=trk.flower.weights_deferred,
                        reused=trk.flower.source_features_reused))
        return out
    trk.flower.compute_flow = compute_flow
    return conf, trk


@torch.no_grad()
def test_tracker_warm_start_over_a_run_of_lost_frames(monkeypatch):
    """The sequence and the forcing device of the recorded lost-frame runs (tools/gen_window_golden.py: the re-detection test is
    swapped for one that never passes on chosen frames): frames 1-3 lost, 4 re-detected, 5 lost again."""
    from woft_amd import forward_interpolate
    monkeypatch.setenv("WOFT_FUSED", "1")
    Hh, Ww, iters = 128, 160, 4
    sd = synth.make_state_dict(seed=7)
    template = synth.make_template(Hh, Ww, seq_id=4)
    mask = synth.make_init_mask(Hh, Ww)
    frames = [synth.make_frame(template, t) for t in (1, 2, 3, 4, 5, 6)]
    fail = {1, 2, 3, 5}
    never = presets.redetection_by_inliers(1e-6, 0.999)
    runs = {}
    for cfg in ("WOFT_warmstart.py", "WOFT.py"):
        spy = []
        conf, trk = _tracker(cfg, sd, iters, spy)
        assert trk.warm_start_local == (cfg == "WOFT_warmstart.py") and trk.warm_start_iters is None
        normal = conf.redet_success_fn
        trk.init(template, mask)
        res = []
        for i, f in enumerate(frames):
            trk.C.redet_success_fn = never if i in fail else normal
            trk._fused = trk._fused_specs()
            n0 = len(spy)
            Hc, m = trk.track(f)
            res.append((np.asarray(Hc, np.float64), m, spy[n0:], trk._warm is None))
        runs[cfg] = res
    warm, cold = runs["WOFT_warmstart.py"], runs["WOFT.py"]
    for i, (H, m, calls, carry_empty) in enumerate(warm):
        assert np.all(np.isfinite(H)) and np.all(np.isfinite(cold[i][0])), i
        assert bool(m.lost) == (i in fail) and bool(cold[i][1].lost) == (i in fail), i
        local = [c for c in calls if c["local"]]
        assert len(local) == (1 if i in fail else 0)
        if i not in fail:
            assert not hasattr(m, "local_warm_started") and carry_empty       # a re-detected frame clears the carry
            continue
        assert m.local_warm_started == (i in (2, 3)), i
        assert cold[i][1].local_warm_started is False
        assert not carry_empty
        if i in (2, 3):
            prev_low = [c for c in warm[i - 1][2] if c["local"]][0]["low"]
            assert torch.equal(local[0]["init"], forward_interpolate(prev_low)), i
            assert local[0]["iters"] is None
            assert local[0]["reused"]                        # src_is_previous_dst honoured together with the flow_init
        else:
            assert local[0]["init"] is None
    # flow_init together with the deferred weight head on the carried mask's region (the default config's sparse weight head)
    assert any(c["deferred"] for i in (2, 3) for c in warm[i][2] if c["local"])
    for i in (0, 1):                # up to and including the first lost frame the two trackers compute the same thing
        assert np.array_equal(warm[i][0], cold[i][0]), i
    for i in (2, 3):
        print(f"frame {i}: warm vs cold template-corner distance {_corner_dist(warm[i][0], cold[i][0], mask):.4f} px")
    torch.cuda.synchronize()


@torch.no_grad()
def test_tracker_warm_start_iters_and_clearing(monkeypatch):
    """`warm_start_iters` reaches the warm-started flows only; init() and a fast-forwarded frame clear the carried flow; a flow that
    ran in the other buffer set is not carried."""
    from types import SimpleNamespace
    monkeypatch.setenv("WOFT_FUSED", "1")
    Hh, Ww = 128, 160
    sd = synth.make_state_dict(seed=7)
    template = synth.make_template(Hh, Ww, seq_id=4)
    mask = synth.make_init_mask(Hh, Ww)
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_warmstart.py")
    conf.flow_config.model, conf.flow_config.iters = sd, 4
    conf.warm_start_iters = 2
    trk = conf.tracker_class(conf)
    normal, never = trk.C.redet_success_fn, presets.redetection_by_inliers(1e-6, 0.999)
    seen = []
    orig = trk.flower.compute_flow

    def compute_flow(src, dst, **kw):
        seen.append((kw.get("flow_init") is not None, kw.get("iters")))
        return orig(src, dst, **kw)
    trk.flower.compute_flow = compute_flow

    def track(t, lost=True):
        trk.C.redet_success_fn = never if lost else normal
        trk._fused = trk._fused_specs()
        return trk.track(synth.make_frame(template, t))[1]
    trk.init(template, mask)
    assert not track(1, lost=False).lost                      # (a re-detected frame first: frame t-1 of the run is not the template)
    flags = [track(t).local_warm_started for t in (2, 3, 4)]
    assert flags == [False, True, True]
    assert [s for s in seen if s[0]] == [(True, 2), (True, 2)] and all(s[1] is None for s in seen if not s[0])
    trk.set_fast_meta(SimpleNamespace(estim_H_current2template=np.eye(3)))
    trk.track(synth.make_frame(template, 5))
    assert trk._warm is None
    assert track(6).local_warm_started is False
    assert trk._warm is not None
    trk.init(template, mask)
    assert trk._warm is None
    # lost straight after init(): frame t-1 IS the pinned template, so the first local flow runs in the template's buffer set and the
    # second, from an ordinary frame, in the other one -- different flow keys, nothing carried; from the third on both ran in the same set
    assert [track(t).local_warm_started for t in (1, 2, 3)] == [False, False, True]
    torch.cuda.synchronize()
