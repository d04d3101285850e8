"""MaskHead ('weighted_masked') on the GPU: the feature-warp kernel against torch's grid_sample, the
operator and the wrapper boundary against the reference's golden outputs (tests/golden/mask_*.npz), the head's stages at
1080p against a CPU restatement, flow / weights unchanged by the head, graph replay, the flow cache."""
import json
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from woft_amd import synth  # noqa: E402


def _flow_config(sd, iters, structure, raft_type="weighted_masked", padding_mode="nopad", small=False, precision="fp32"):
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
    c.padding_mode = padding_mode
    if precision:
        c.precision = precision
    return c


def _epe(a, b):
    d = torch.as_tensor(a).detach().cpu().float() - torch.as_tensor(b).detach().cpu().float()
    e = torch.sqrt((d ** 2).sum(dim=-3))
    return float(e.mean()), float(e.max())


def _sig_err(a, b):
    a, b = torch.as_tensor(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)), torch.as_tensor(np.asarray(b))
    return float((torch.sigmoid(a.float().reshape(-1)) - torch.sigmoid(b.float().reshape(-1))).abs().max())


def _bilinear_sampler(f, coords):
    """The reference's sampler as stated in its contract: pixel coordinates normalised by 2x/(W-1)-1, grid_sample with
    align_corners=True and zero padding.  f (1, C, H, W), coords (N, 2) -> (N, C)."""
    H, W = f.shape[-2:]
    x, y = coords[:, :1], coords[:, 1:]
    grid = torch.cat([2 * x / (W - 1) - 1, 2 * y / (H - 1) - 1], dim=-1).reshape(1, 1, -1, 2)
    return F.grid_sample(f, grid, align_corners=True)[0, :, 0].t()


# ---- kernel ------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("c,cs,ld_out", [(128, 128, 128), (256, 256, 256), (128, 160, 136), (256, 256, 288)])
def test_warp_features_vs_grid_sample(c, cs, ld_out):
    from woft_amd import ops
    rs = np.random.RandomState(c + cs + ld_out)
    h, w = 13, 17
    f = torch.from_numpy(rs.randn(h * w, cs).astype(np.float32))
    pts = [(0, 0), (w - 1, h - 1), (3, 5), (w - 1, 0), (0, h - 1), (7.5, 6.25), (w - 1.25, h - 1.5),    # integers, edges, inside
           (-0.5, 3.0), (w - 0.5, 4.0), (5.0, -0.75), (6.0, h - 0.25), (-0.999, -0.999), (w - 0.001, h - 0.001),  # just outside
           (-1.0, 2.0), (w, 3.0), (-1.5, -1.5), (w + 0.5, h + 0.5),                                       # a corner away / beyond
           (-1e4, 5.0), (5.0, 3e6), (-3e9, -3e9), (1e30, 2.0), (-7.25, 40.5)]                              # far outside, negative
    rnd = np.stack([rs.uniform(-2, w + 1, 300), rs.uniform(-2, h + 1, 300)], 1)
    coords = torch.from_numpy(np.concatenate([np.array(pts, np.float64), rnd]).astype(np.float32))
    n = coords.shape[0] - 1                                                    # (not a multiple of 4)
    coords = coords[:n].contiguous()
    ref = _bilinear_sampler(f[:, :c].reshape(1, h, w, c).permute(0, 3, 1, 2).contiguous(), coords)
    src = ops.Act(f.cuda(), 1, h, w, c)
    out = ops.Act(torch.full((n, ld_out), 12345.0, device="cuda"), n, 1, 1, c)
    ops.warp_features(src, coords.cuda(), out)
    torch.cuda.synchronize()
    got = out.t.cpu()
    err = (got[:, :c] - ref).abs() / (1 + ref.abs())
    assert float(err.max()) <= 1e-5, (float(err.max()), int(err.max(1).values.argmax()))
    assert bool((got[:, c:] == 12345.0).all())                                  # channels beyond c untouched
    assert bool((got[17:21, :c] == 0).all())                                    # far outside: exact zeros


# ---- operator vs the reference's golden --------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("name", ["full", "small"])
@pytest.mark.parametrize("precision,epe_mean,epe_max,wtol,mtol", [("fp32", 1e-3, 1e-2, 1e-4, 1e-4), ("bf16x3", 1e-3, 1e-2, 1e-4, 1e-4),
                                                                  ("bf16", 5e-2, 0.5, 5e-3, 5e-3)])
def test_operator_vs_golden(golden_dir, name, precision, epe_mean, epe_max, wtol, mtol):
    g = np.load(golden_dir / "mask_head_128x160_it4.npz")
    small, st = bool(int(g[f"{name}_small"])), json.loads(str(g[f"{name}_structure"]))
    sd = synth.make_state_dict(seed=int(g[f"{name}_seed"]), small=small, mask_head_structure=st)
    fc = _flow_config(sd, int(g["iters"]), st, small=small, precision=precision)
    flower = fc.of_class(fc)
    flow, w, m = flower.compute_flow(g[f"{name}_img1"], g[f"{name}_img2"], mode="flow", do_sigmoid=False)
    torch.cuda.synchronize()
    assert tuple(flow.shape) == (2, 128, 160) and tuple(w.shape) == (1, 128, 160) and tuple(m.shape) == (1, 128, 160)
    mean, mx = _epe(flow, g[f"{name}_flow_up"][0])
    assert mean < epe_mean and mx < epe_max, (mean, mx)
    assert _sig_err(w, g[f"{name}_w_up"]) < wtol
    assert _sig_err(m, g[f"{name}_mask_up"]) < mtol, _sig_err(m, g[f"{name}_mask_up"])
    plan = next(iter(flower.engine._plans.values()))
    assert _sig_err(plan.mh_low, g[f"{name}_mask_low"]) < mtol


@torch.no_grad()
def test_mixed_precision_runs_the_head_in_fp32_class_arithmetic(golden_dir):
    """fp16 (`mixed_precision`): the reference runs the MaskHead outside autocast -- here bf16x3, the weight head's rule."""
    g = np.load(golden_dir / "mask_head_128x160_it4.npz")
    st = json.loads(str(g["full_structure"]))
    sd = synth.make_state_dict(seed=int(g["full_seed"]), mask_head_structure=st)
    fc = _flow_config(sd, int(g["iters"]), st, precision=None)
    fc.class_params.mixed_precision = True
    flower = fc.of_class(fc)
    assert flower.precision == "fp16" and flower.engine.prec_wh == "bf16x3"
    flow, w, m = flower.compute_flow(g["full_img1"], g["full_img2"], mode="flow")
    torch.cuda.synchronize()
    plan = next(iter(flower.engine._plans.values()))
    assert all(p.precision == 1 for p in plan.prog_mh)
    mean, mx = _epe(flow, g["full_flow_up"][0])
    assert mean < 1e-2 and mx < 0.1, (mean, mx)
    assert _sig_err(w, g["full_w_up"]) < 1e-3 and _sig_err(m, g["full_mask_up"]) < 1e-3


# ---- wrapper boundary vs the reference wrapper's golden ----------------------------------------------------------------
@torch.no_grad()
def test_wrapper_boundary_vs_golden(golden_dir):
    g = np.load(golden_dir / "mask_wrapper_128x160_it4.npz")
    st = json.loads(str(g["structure"]))
    sd = synth.make_state_dict(seed=int(g["seed"]), mask_head_structure=st)
    a, b = g["img1"], g["img2"]
    logit_close = lambda x, ref: float((np.abs(np.asarray(x) - ref) / (1 + np.abs(ref))).max()) < 4e-4
    flower = (lambda c: c.of_class(c))(_flow_config(sd, int(g["iters"]), st))
    src, dst, w, m = flower.compute_flow(a, b, mode="TC", do_sigmoid=True)
    torch.cuda.synchronize()
    assert src.dtype == torch.int64 and tuple(src.shape) == (2, 128 * 160)
    assert dst.dtype == torch.float32 and tuple(dst.shape) == (2, 128 * 160)
    assert w.dtype == m.dtype == torch.float32 and tuple(w.shape) == tuple(m.shape) == (1, 128 * 160) and m.is_cuda
    assert np.abs(dst.cpu().numpy() - g["dst"]).max() < 1e-2
    assert np.abs(w.cpu().numpy() - g["w"]).max() < 1e-4
    assert logit_close(m.cpu().numpy(), g["m"])                 # do_sigmoid: the weights only -- the mask stays logits
    flow, wl, mf = flower.compute_flow(a, b, mode="flow", do_sigmoid=False)
    torch.cuda.synchronize()
    assert tuple(flow.shape) == (2, 128, 160) and tuple(wl.shape) == tuple(mf.shape) == (1, 128, 160)
    assert logit_close(wl.cpu().numpy().reshape(1, -1), g["w_logit"].reshape(1, -1))
    assert logit_close(mf.cpu().numpy().reshape(1, -1), g["m"])
    res = flower.compute_flow(a, b, mode="flow", numpy_out=True)
    assert len(res) == 3 and all(isinstance(r, np.ndarray) for r in res) and res[2].shape == (1, 128, 160)
    res = flower.compute_flow(a, b, mode="TC", numpy_out=True)
    assert len(res) == 4 and all(isinstance(r, np.ndarray) for r in res) and res[3].shape == (1, 128 * 160)
    assert logit_close(res[3], g["m"])
    b1 = flower.compute_flow(a, b, mode="TC", borrow=True)[3]
    b2 = flower.compute_flow(a, b, mode="TC", borrow=True)[3]
    assert b1.data_ptr() == b2.data_ptr()                        # borrow: the provider's own mask buffer
    c = _flow_config(sd, int(g["iters"]), st, padding_mode="RAFT")
    s2, d2, w2, m2 = c.of_class(c).compute_flow(a[:125, :157].copy(), b[:125, :157].copy(), mode="TC", do_sigmoid=True)
    torch.cuda.synchronize()
    assert tuple(m2.shape) == (1, 125 * 157) and logit_close(m2.cpu().numpy(), g["m_pad"])
    c = _flow_config(sd, int(g["iters"]), st, padding_mode="crop")
    s4, d4, w4, m4 = c.of_class(c).compute_flow(a[:, :157].copy(), b[:, :157].copy(), mode="TC", do_sigmoid=True)
    torch.cuda.synchronize()
    assert tuple(m4.shape) == (1, 128 * 152) and logit_close(m4.cpu().numpy(), g["m_crop"])


# ---- the head's stages at 1080p against a CPU restatement -------------------------------------------------------------
def _convex_up(x, up_mask):
    """x (1, 1, h, w), up_mask (1, 576, h, w) -> (1, 1, 8h, 8w): RAFT's convex upsampling (softmax over the 3x3 neighbours)."""
    _, _, h, w = x.shape
    m = torch.softmax(up_mask.view(1, 1, 9, 8, 8, h, w), dim=2)
    nb = F.unfold(8 * x, [3, 3], padding=1).view(1, 1, 9, 1, 1, h, w)
    return (m * nb).sum(dim=2).permute(0, 1, 4, 2, 5, 3).reshape(1, 1, 8 * h, 8 * w)


@torch.no_grad()
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_stages_1080p_vs_cpu_restatement(precision):
    from woft_amd.engine import RaftEngine
    st = [(128, 3), (64, 5)]
    sd = synth.make_state_dict(seed=5, mask_head_structure=st)
    H, W = 1080, 1920
    a = synth.make_template(H, W, seq_id=2)
    b = synth.make_frame(a, 2)
    eng = RaftEngine(sd, precision=precision, corr="otf", mask_head=True)
    plan = eng.plan(H, W)
    plan.load_image(0, torch.from_numpy(a).cuda(), 0, 0)
    plan.load_image(1, torch.from_numpy(b).cuda(), 0, 0)
    plan.encode_source()
    mout = torch.zeros(1, H * W, device="cuda")
    plan.flow(3, (0, 0), H, W, dst=torch.zeros(2, H * W, device="cuda"), mout=mout)
    torch.cuda.synchronize()
    hf, wf = plan.hf, plan.wf
    f1, f2 = plan.f1.nchw().cpu(), plan.f2act[0].nchw().cpu()
    coords = plan.coords.cpu()
    up_mask = plan.mask.t[:, :576].cpu().reshape(1, hf, wf, 576).permute(0, 3, 1, 2)
    warped = _bilinear_sampler(f2, coords).t().reshape(1, -1, hf, wf)
    assert float((plan.mh_warped.nchw().cpu() - warped).abs().max()) <= 1e-5 * (1 + float(warped.abs().max()))
    x = torch.cat([f1, warped], 1)
    for i, (c, k) in enumerate(st):
        x = F.relu(F.conv2d(x, sd[f"mask_head.net.{2 * i}.weight"], sd[f"mask_head.net.{2 * i}.bias"], padding=k // 2))
    low = F.conv2d(x, sd[f"mask_head.net.{2 * len(st)}.weight"], sd[f"mask_head.net.{2 * len(st)}.bias"])
    up = (_convex_up(low, up_mask) / 8).reshape(1, -1)
    got_low = plan.mh_low.cpu().reshape(1, 1, hf, wf)
    if precision == "fp32":
        assert float(((got_low - low).abs() / (1 + low.abs())).max()) <= 1e-4
        assert float(((mout.cpu() - up).abs() / (1 + up.abs())).max()) <= 1e-4
    assert _sig_err(got_low, low) <= 1e-4 and _sig_err(mout, up) <= 1e-4


# ---- the head leaves flow and weights alone ------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("precision,small", [("bf16x3", False), ("fp32", False), ("bf16x3", True)])
def test_flow_and_weights_bit_identical_to_weighted(precision, small):
    st = [(96, 3), 32]
    sd_w = synth.make_state_dict(seed=6, small=small)
    sd_m = synth.make_state_dict(seed=6, small=small, mask_head_structure=st)
    h, w = 136, 200
    a = synth.make_template(h, w, seq_id=6)
    b = synth.make_frame(a, 3)
    cw = _flow_config(sd_w, 4, None, raft_type="weighted", padding_mode="RAFT", small=small, precision=precision)
    cm = _flow_config(sd_m, 4, st, padding_mode="RAFT", small=small, precision=precision)
    fw, ww = cw.of_class(cw).compute_flow(a, b, mode="flow")
    fm, wm, mm = cm.of_class(cm).compute_flow(a, b, mode="flow")
    torch.cuda.synchronize()
    assert torch.equal(fw, fm) and torch.equal(ww, wm)
    assert bool(torch.isfinite(mm).all()) and float(mm.abs().max()) > 0


# ---- graph replay, both plan slots -------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("precision,small", [("bf16x3", False), ("fp32", True)])
def test_graph_replay_matches_eager(precision, small):
    st = [(64, 3)]
    sd = synth.make_state_dict(seed=12, small=small, mask_head_structure=st)
    h, w = 136, 200
    a = synth.make_template(h, w, seq_id=4)
    frames = [synth.make_frame(a, t) for t in (1, 2, 3, 4, 5)]
    outs = {}
    for graph in (False, True):
        c = _flow_config(sd, 4, st, padding_mode="RAFT", small=small, precision=precision)
        c.graph = graph
        prov = c.of_class(c)
        assert prov.use_graph == graph
        prov.pin_source(a)
        res = []
        for k, f in enumerate(frames):
            # pinned source (plan slot 0), then flows between two frames (slot 1), three calls each: eager, capture, replay
            s_img = a if k < 3 else frames[k - 3]
            src, dst, wt, m = prov.compute_flow(s_img, f, mode="TC", do_sigmoid=True)
            res.append((dst.cpu().numpy().copy(), wt.cpu().numpy().copy(), m.cpu().numpy().copy()))
        for k in range(3):
            _, dst, wt, m = prov.compute_flow(frames[k], frames[k + 1], mode="TC", do_sigmoid=True)
            res.append((dst.cpu().numpy().copy(), wt.cpu().numpy().copy(), m.cpu().numpy().copy()))
        outs[graph] = res
        if graph:
            for plan in prov.engine._plans.values():
                assert any(g is not None for g in plan._graphs.values())       # replayed in both slots
            assert len(prov.engine._plans) == 2
    for r0, r1 in zip(outs[False], outs[True]):
        for x0, x1 in zip(r0, r1):
            assert np.array_equal(x0, x1)


# ---- the flow cache ------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_cached_flow_is_skipped_and_the_mask_computed(tmp_path, caplog):
    h, w = 128, 160
    rng = np.random.RandomState(5)
    d = tmp_path / "ds" / "seq"
    d.mkdir(parents=True)
    np.savez(d / "7-8.npz", half_flow=(rng.randn(2, h, w) * 3).astype(np.float16),
             half_weights=rng.randn(1, h, w).astype(np.float16))
    st = [(64, 3)]
    c = _flow_config(synth.make_state_dict(seed=3, mask_head_structure=st), 2, st)
    c.flow_cache_dir = tmp_path
    prov = c.of_class(c)
    img = synth.make_template(h, w, seq_id=1)
    img2 = synth.make_frame(img, 1)
    ref = prov.compute_flow(img, img2, mode="TC", numpy_out=True)
    with caplog.at_level(logging.WARNING, logger="woft_amd.flow_provider"):
        for _ in range(2):
            got = prov.compute_flow(img, img2, mode="TC", src_img_identifier=("ds", "seq", 7), numpy_out=True)
            assert len(got) == 4
            for x, y in zip(ref, got):
                assert np.array_equal(x, y)
    assert sum("flow cache holds no visibility mask" in r.getMessage() for r in caplog.records) == 1
