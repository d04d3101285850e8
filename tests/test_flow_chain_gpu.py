"""Flow sampling, chaining and the forward-backward check on the GPU.

Kernels: woft_sample_bilinear against the reference's own outputs (tests/golden/flow_interp.npz) and the numpy restatement, as
bits; woft_flow_chain / woft_flow_fb against the fp64 restatement (tests/flow_chain_host.py) within bounds derived from the
formulas.  Provider: compute_flow_fb against its parts.  Tracker: `fb_check` leaves the forward flow alone, fills the meta fields
and fits what the public pieces give when run by hand, in both solver back ends."""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flow_chain_host as FH  # noqa: E402
from woft_amd import ops, presets, synth  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
EPS = 2.0 ** -24
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def gold():
    return np.load(ROOT / "tests" / "golden" / "flow_interp.npz")


# ---- the reference sampler ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hand_5x7", "rand_33x65", "row_1x9", "col_9x1"])
def test_sampler_equals_the_reference_as_bits(gold, case):
    from pytracking.utils.interpolation import bilinear_interpolate_torch, flow_warp_coords
    data, x, y = (gold[f"{case}_{k}"] for k in ("data", "x", "y"))
    out = ops.sample_bilinear(cuda(data), cuda(x), cuda(y)).cpu().numpy()
    assert np.array_equal(bits(out), bits(gold[f"{case}_interp"]))
    # the shim import path, host tensors in and out (copied to the device and back)
    host = bilinear_interpolate_torch(torch.from_numpy(data), torch.from_numpy(x), torch.from_numpy(y))
    assert not host.is_cuda and host.dtype == torch.float32 and np.array_equal(bits(host.numpy()), bits(gold[f"{case}_interp"]))
    if data.shape[0] == 2:
        for dev in ("cpu", "cuda"):
            warped = flow_warp_coords(torch.from_numpy(np.stack([x, y])).to(dev), torch.from_numpy(data).to(dev))
            assert warped.device.type == dev and tuple(warped.shape) == (2, x.size)
            assert np.array_equal(bits(warped.cpu().numpy()), bits(gold[f"{case}_warp"]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_sampler_equals_the_restatement_as_bits(gold, n):
    data = gold["rand_33x65_data"]
    rs = np.random.RandomState(n)
    x, y = rs.uniform(-3, 68, n).astype(np.float32), rs.uniform(-3, 36, n).astype(np.float32)
    x[::5], y[::7] = np.round(x[::5]), np.round(y[::7])
    out = torch.full((2, n + 8), 7.0, device="cuda")
    got = ops.sample_bilinear(cuda(data), cuda(x), cuda(y), out=out.reshape(-1)[:2 * n].view(2, n)).cpu().numpy()
    assert np.array_equal(bits(got), bits(FH.sample_ref32(data, x, y)))
    assert (out.reshape(-1)[2 * n:] == 7.0).all()                          # nothing written past the (C, N) block


def test_sampler_non_finite_and_huge_coordinates(gold):
    """Values with defined results (the kernel is safe by the construction of its index, not by this test): a NaN or infinite
    coordinate gives NaN in every channel -- a NaN enters all four weights; an infinite one makes weights of both signs, inf - inf.
    A coordinate of 3e38 beyond the last column gives 0 where the other coordinate makes the result defined: on the last row every
    weight is a product with (y1 - y) = (y - y0) = 0, and at y = -0.5 (both corners clamped to row 0) the four weights are
    -+1.5e38 on ONE pixel a, ((-A + A) + A) - A = 0 exactly for |a| <= 1 (no overflow)."""
    data = np.clip(gold["rand_33x65_data"], -1.0, 1.0)
    h, w = data.shape[1:]
    bad = [NAN, INF, -INF]
    x = np.array(bad + [3.5] * 3 + bad, np.float32)
    y = np.array([2.5] * 3 + bad + bad[::-1], np.float32)
    out = ops.sample_bilinear(cuda(data), cuda(x), cuda(y)).cpu().numpy()
    assert np.isnan(out).all()
    assert np.array_equal(np.isnan(FH.sample_ref32(data, x, y)), np.isnan(out))
    big = np.float32(3e38)
    x = np.array([big, big, 10.0, -0.5, big, -big], np.float32)
    y = np.array([h - 1, -0.5, big, big, 5.0, 5.0], np.float32)
    out = ops.sample_bilinear(cuda(data), cuda(x), cuda(y)).cpu().numpy()
    assert np.array_equal(bits(out), bits(FH.sample_ref32(data, x, y)))
    assert not out[:, :4].any() and np.isfinite(out).all()


# ---- chain and fb against the fp64 restatement -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fields():
    """Per shape: the two fields, their device copies and the fp64 references (computed once, read by both tests)."""
    out = {}
    for h, w in FH.SHAPES:
        fwd, bwd = FH.make_fields(h, w)
        out[(h, w)] = dict(fwd=fwd, bwd=bwd, dfwd=cuda(fwd), dbwd=cuda(bwd), chain=FH.chain64(fwd, bwd),
                           fb=FH.fb64(fwd, bwd, 0.01, 0.5))
    return out


@pytest.mark.parametrize("shape", FH.SHAPES)
def test_chain_against_fp64(fields, shape):
    """|fac - fac64| <= 8 eps * (max |tap| of the pixel) + eps * |fac64|, eps = 2^-24: the four products and three sums of the
    sampler (weights in [0, 1], each themselves rounded) and the final add."""
    from woft_amd import chain_flow
    c = fields[shape]
    fac64, valid, tapmax = c["chain"]
    got = ops.flow_chain(c["dfwd"], c["dbwd"]).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(fac64)) and np.array_equal(np.isnan(got[0]), ~valid)
    diff = np.abs(got.astype(np.float64) - fac64)[:, valid]
    bound = (8 * EPS * tapmax[None] + EPS * np.abs(fac64))[:, valid]
    print(f"chain {shape}: {valid.sum()} of {valid.size} valid, max |diff| {diff.max():.3e}, max diff / bound {(diff / bound).max():.3f}")
    assert (diff <= bound).all()
    # the public function: (2, H, W) and (B, 2, H, W), host and device, the same bits
    for a, b in ((c["dfwd"], c["dbwd"]), (torch.from_numpy(c["fwd"]), torch.from_numpy(c["bwd"]))):
        assert np.array_equal(bits(chain_flow(a, b).cpu().numpy()), bits(got))
        both = chain_flow(torch.stack([a, b]), torch.stack([b, a]))
        assert both.device == a.device and np.array_equal(bits(both[0].cpu().numpy()), bits(got))
        assert np.array_equal(bits(both[1].cpu().numpy()), bits(ops.flow_chain(c["dbwd"], c["dfwd"]).cpu().numpy()))


@pytest.mark.parametrize("shape", FH.SHAPES)
def test_fb_against_fp64(fields, shape):
    """|err - err64| <= 16 eps * (M + err64), M the largest flow magnitude in both fields; ok equals the fp64 verdict wherever
    |e2 - bound| > 1e-4 * bound in fp64 (at most 0.5 % of the pixels may be left out by that margin)."""
    from woft_amd import fb_consistency
    c = fields[shape]
    err64, ok64, e2, bound, valid = c["fb"]
    err, ok = ops.flow_fb(c["dfwd"], c["dbwd"], 0.01, 0.5)
    err, ok = err.cpu().numpy(), ok.cpu().numpy()
    assert np.array_equal(np.isposinf(err), ~valid) and np.isfinite(err[valid]).all() and not np.isnan(err).any()
    assert set(np.unique(ok)) <= {0.0, 1.0} and not ok[~valid].any()
    M = max(np.hypot(c["fwd"][0].astype(np.float64), c["fwd"][1]).max(), np.hypot(c["bwd"][0].astype(np.float64), c["bwd"][1]).max())
    diff = np.abs(err[valid].astype(np.float64) - err64[valid])
    lim = 16 * EPS * (M + err64[valid])
    decided = ~valid | (np.abs(e2 - bound) > 1e-4 * bound)
    left_out = int((~decided).sum())
    print(f"fb {shape}: {valid.sum()} of {valid.size} valid, {int(ok64.sum())} ok, max |err diff| {diff.max():.3e}, "
          f"max diff / bound {(diff / lim).max():.3f}, {left_out} pixels within the verdict margin")
    assert (diff <= lim).all()
    assert left_out <= 0.005 * valid.size, f"{left_out} of {valid.size} pixels within 1e-4 of the bound"
    assert np.array_equal(ok[decided] == 1.0, ok64[decided]), f"{left_out} pixels left out"
    # either output alone, and the public function in both layouts on both devices
    only_err, none = ops.flow_fb(c["dfwd"], c["dbwd"], 0.01, 0.5, want_ok=False)
    none2, only_ok = ops.flow_fb(c["dfwd"], c["dbwd"], 0.01, 0.5, want_err=False)
    assert none is None and none2 is None
    assert np.array_equal(bits(only_err.cpu().numpy()), bits(err)) and np.array_equal(only_ok.cpu().numpy(), ok)
    h, w = shape
    for a, b in ((c["dfwd"], c["dbwd"]), (torch.from_numpy(c["fwd"]), torch.from_numpy(c["bwd"]))):
        e1, o1 = fb_consistency(a, b)
        assert tuple(e1.shape) == tuple(o1.shape) == (1, h, w) and e1.device == a.device
        assert np.array_equal(bits(e1.cpu().numpy()[0]), bits(err)) and np.array_equal(o1.cpu().numpy()[0], ok)
        e2_, o2 = fb_consistency(torch.stack([a, a]), torch.stack([b, b]), alpha=0.01, beta=0.5)
        assert tuple(e2_.shape) == (2, 1, h, w) and np.array_equal(bits(e2_.cpu().numpy()[1, 0]), bits(err))
        assert np.array_equal(o2.cpu().numpy()[0, 0], ok)


def test_rows_beyond_one_grid_pass():
    """More than 65535 * 4 rows: the per-pixel kernels walk the rows a second time (grid-stride loop).  Same bounds as above."""
    h, w = 65535 * 4 + 9, 2
    rs = np.random.RandomState(5)
    fwd = np.stack([rs.uniform(-0.6, 0.6, (h, w)), rs.uniform(-2.5, 2.5, (h, w))]).astype(np.float32)
    bwd = (-fwd + rs.normal(0, 0.4, fwd.shape)).astype(np.float32)
    dfwd, dbwd = cuda(fwd), cuda(bwd)
    fac64, valid, tapmax = FH.chain64(fwd, bwd)
    got = ops.flow_chain(dfwd, dbwd).cpu().numpy()
    assert np.array_equal(np.isnan(got[0]), ~valid) and np.array_equal(np.isnan(got[1]), ~valid)
    assert 0.2 < valid.mean() < 0.9 and valid[-9:].any() and (~valid[-9:]).any()
    diff = np.abs(got.astype(np.float64) - fac64)[:, valid]
    assert (diff <= (8 * EPS * tapmax[None] + EPS * np.abs(fac64))[:, valid]).all()
    err64, ok64, e2, bound, _ = FH.fb64(fwd, bwd, 0.01, 0.5)
    err, ok = (t.cpu().numpy() for t in ops.flow_fb(dfwd, dbwd, 0.01, 0.5))
    assert np.array_equal(np.isposinf(err), ~valid)
    M = max(np.hypot(fwd[0].astype(np.float64), fwd[1]).max(), np.hypot(bwd[0].astype(np.float64), bwd[1]).max())
    assert (np.abs(err[valid].astype(np.float64) - err64[valid]) <= 16 * EPS * (M + err64[valid])).all()
    decided = ~valid | (np.abs(e2 - bound) > 1e-4 * bound)
    left_out = int((~decided).sum())
    assert left_out <= 0.005 * valid.size and np.array_equal(ok[decided] == 1.0, ok64[decided]), left_out
    assert ok64[-9:].any() or ok64[-40:].any()


def test_fb_non_finite_flows_and_dtypes():
    from woft_amd import fb_consistency
    fwd = np.zeros((2, 6, 8), np.float32)
    bwd = np.zeros((2, 6, 8), np.float32)
    fwd[0, 1, 1] = NAN              # a NaN forward flow: nowhere to land
    fwd[1, 2, 2] = INF
    bwd[0, 0, 0] = NAN              # a NaN reverse flow under a valid landing point (the first pixel: no other pixel taps it)
    fwd[0, 4, 4] = 3e38
    err, ok = ops.flow_fb(cuda(fwd), cuda(bwd), 0.0, 0.0)
    err, ok = err.cpu().numpy(), ok.cpu().numpy()
    for y, x in ((1, 1), (2, 2), (4, 4)):
        assert np.isposinf(err[y, x]) and ok[y, x] == 0.0
    assert np.isnan(err[0, 0]) and ok[0, 0] == 0.0
    rest = np.ones((6, 8), bool)
    rest[[1, 2, 0, 4], [1, 2, 0, 4]] = False
    assert (err[rest] == 0.0).all() and (ok[rest] == 1.0).all()      # (alpha = beta = 0: 0 <= 0 holds)
    fac = ops.flow_chain(cuda(fwd), cuda(bwd)).cpu().numpy()
    for y, x in ((1, 1), (2, 2), (4, 4)):
        assert np.isnan(fac[:, y, x]).all()                            # an invalid landing point: NaN in both planes
    assert np.isnan(fac[0, 0, 0]) and fac[1, 0, 0] == 0.0              # a NaN tap stays in its own plane
    assert (fac[:, rest] == 0.0).all()
    e16, o16 = fb_consistency(torch.from_numpy(fwd).double(), torch.from_numpy(bwd).double())
    assert e16.dtype == o16.dtype == torch.float64 and not e16.is_cuda     # (computed in fp32, cast back)


# ---- provider -------------------------------------------------------------------------------------------------------------------
ITERS = 3


def _flow_config(raft_type, padding_mode):
    from pytracking.utils.config import load_config
    fc = load_config(ROOT / "pytracking" / "optical_flow" / "configs" / "v2_SNOB_large_g05_RAFT.py")
    fc.model = synth.make_state_dict(seed=7, weighted=raft_type != "orig")
    fc.raft_type, fc.iters, fc.padding_mode, fc.precision = raft_type, ITERS, padding_mode, "bf16x3"
    return fc


@pytest.mark.parametrize("padding_mode,hw", [("nopad", (128, 160)), ("RAFT", (130, 163))])
@pytest.mark.parametrize("raft_type", ["orig", "weighted"])
def test_compute_flow_fb_equals_its_parts(raft_type, padding_mode, hw):
    from woft_amd import fb_consistency
    h, w = hw
    fc = _flow_config(raft_type, padding_mode)
    prov = fc.of_class(fc)
    a = synth.make_template(h, w, seq_id=3)
    b = synth.make_frame(a, 2)
    fwd, bwd, err, ok = prov.compute_flow_fb(a, b, alpha=0.02, beta=0.25)
    assert [tuple(t.shape) for t in (fwd, bwd, err, ok)] == [(2, h, w), (2, h, w), (1, h, w), (1, h, w)]
    f1 = prov.compute_flow(a, b, mode="flow")
    f2 = prov.compute_flow(b, a, mode="flow")
    assert (f1[1] is None) == (raft_type == "orig")
    assert torch.equal(fwd.view(torch.int32), f1[0].view(torch.int32)) and torch.equal(bwd.view(torch.int32), f2[0].view(torch.int32))
    assert fwd.data_ptr() != f1[0].data_ptr() and float(fwd.abs().max()) > 0 and not torch.equal(fwd, bwd)
    e, o = fb_consistency(f1[0], f2[0], alpha=0.02, beta=0.25)
    assert torch.equal(err.view(torch.int32), e.view(torch.int32)) and torch.equal(ok, o)
    n_ok = int(ok.sum())
    print(f"{raft_type} {padding_mode}: {n_ok} of {h * w} pixels consistent, {int(torch.isinf(err).sum())} leave the frame")
    # the tensors are the caller's own: another flow at this size leaves them alone; numpy_out gives the same values
    keep = fwd.clone()
    out = prov.compute_flow_fb(b, a, alpha=0.02, beta=0.25, numpy_out=True)
    assert torch.equal(fwd, keep) and all(isinstance(t, np.ndarray) for t in out)
    assert np.array_equal(bits(out[0]), bits(bwd.cpu().numpy())) and np.array_equal(bits(out[1]), bits(fwd.cpu().numpy()))
    with pytest.raises(ValueError, match="alpha and beta"):
        prov.compute_flow_fb(a, b, alpha=-1.0)


# ---- tracker --------------------------------------------------------------------------------------------------------------------
HH, WW = 128, 160
ALPHA, BETA = 0.05, 2.0             # (seeded random weights give an arbitrary flow: loose constants keep some correspondences)


@pytest.fixture(scope="module")
def seq():
    template = synth.make_template(HH, WW, seq_id=5)
    return dict(template=template, mask=synth.make_init_mask(HH, WW), frames=[synth.make_frame(template, t) for t in (1, 2, 3)])


def _sobol_subsampler_any_weights(coords_a, coords_b, weights, post_weights):
    """presets.sobol_subsampler(500) for a network without weights: the preset (as the reference's config) asserts a weight
    tensor, which raft_type 'orig' does not have."""
    n = coords_a.shape[1]
    if n <= 500:
        return coords_a, coords_b, weights, post_weights
    keep = np.zeros(n) > 0
    keep[np.round(n * presets.sobol_points(500)).astype(np.int32)] = True
    return coords_a[:, keep], coords_b[:, keep], (None if weights is None else weights[:, keep]), post_weights


def _tracker(monkeypatch, raft_type, **keys):
    from pytracking.utils.config import load_config
    monkeypatch.setenv("WOFT_FUSED", "1")
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
    conf.flow_config = _flow_config(raft_type, "nopad")
    if raft_type == "orig":
        conf.subsampler_fn = _sobol_subsampler_any_weights
    for k, v in keys.items():
        setattr(conf, k, v)
    trk = conf.tracker_class(conf)
    assert (trk._fused is not None) == (raft_type == "weighted")
    return trk, conf


def _record_solves(trk):
    log, inner = [], trk._solve

    def solve(src_xy, dst_xy, w, grid, frame_hw, src_mask_u8, dst_valid_u8, bounds, judge, vis=None):
        rec = dict(src=src_xy, dst=dst_xy.clone(), w=None if w is None else w.clone(), vis=None if vis is None else vis.clone(),
                   grid=grid, frame_hw=tuple(frame_hw), tmask=src_mask_u8.clone(),
                   pw=None if dst_valid_u8 is None else dst_valid_u8.clone(), bounds=bounds, judge=judge, H=None, n_kept=None)
        log.append(rec)
        try:
            fit = inner(src_xy, dst_xy, w, grid, frame_hw, src_mask_u8, dst_valid_u8, bounds, judge, vis=vis)
        finally:
            rec["n_kept"] = trk.n_kept
        rec["H"] = fit.H.copy()
        return fit
    trk._solve = solve
    return log


def _fit_by_hand(conf, rec, vis, device_backend):
    """One solve from the public pieces: the gate at 0.5 on `vis` in the select / flags kernel, then the config's estimator."""
    Hh, Ww = rec["frame_hw"]
    if device_backend:
        n = Hh * Ww
        pa, pb, wo = torch.empty(1024, 2, device="cuda"), torch.empty(1024, 2, device="cuda"), torch.empty(1024, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        u = cuda(presets.sobol_points(500).astype(np.float32))
        ops.tc_select_vis(rec["dst"], rec["w"], rec["tmask"], rec["pw"], Hh, Ww, rec["bounds"], u, vis, "gate", 0.5,
                          ops.tc_select_ws(n), pa, pb, wo, cnt)
        Hout, status = torch.empty(9, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.hfit(pa, pb, wo, Hout, status, count=cnt[0:1])
        return Hout.cpu().numpy().astype(np.float64).reshape(3, 3), int(cnt[1])
    keep = ops.tc_flags_vis(rec["dst"] if rec["bounds"] else None, rec["tmask"], rec["pw"], Hh, Ww, rec["bounds"], vis, "gate", 0.5)
    src, dst = rec["src"][:, keep], rec["dst"][:, keep]
    w = None if rec["w"] is None else rec["w"][:, keep]
    n_kept = int(src.shape[1])
    if rec["judge"]:
        src = src.float()
    src, dst, w, _ = conf.subsampler_fn(src, dst, w, None)
    Hm = conf.H_estimator(dst.T[None], src.float().T[None], w)
    return Hm.float().detach().cpu().numpy()[0].astype(np.float64), n_kept


@pytest.mark.parametrize("raft_type", ["orig", "weighted"])
def test_tracker_with_fb_check(seq, monkeypatch, raft_type):
    """'orig' runs the callable back end, 'weighted' the device back end.  Frame 0 is forced lost (as tests/test_tracker_gpu.py
    forces one): its global AND local stage both run from the template's pose on the same images in the run with and the run
    without the key, so the two runs' forward flows can be compared stage by stage; later frames check the meta fields and the fit."""
    from woft_amd import fb_consistency
    device_backend = raft_type == "weighted"
    never = presets.redetection_by_inliers(1e-6, 0.999)
    runs = {}
    for name, keys in (("fb", dict(fb_check="gate", fb_alpha=ALPHA, fb_beta=BETA)), ("plain", dict(sparse_weight_head=False))):
        trk, conf = _tracker(monkeypatch, raft_type, **keys)
        normal = conf.redet_success_fn
        log = _record_solves(trk)
        trk.init(seq["template"], seq["mask"])
        metas = []
        for i, f in enumerate(seq["frames"]):
            trk.C.redet_success_fn = never if i == 0 else normal
            trk._fused = trk._fused_specs()
            Hc, meta = trk.track(f)
            metas.append((Hc, meta))
        runs[name] = (trk, conf, log, metas)
    trk, conf, log, metas = runs["fb"]
    _, _, plog, pmetas = runs["plain"]
    assert "forward-backward check gate" in trk.solver_decision and trk.solver_decision.startswith(
        "device back end" if device_backend else "callable back end")
    # meta fields
    m0 = metas[0][1]
    assert m0.fb_check == "gate" and m0.solver_decision == trk.solver_decision and m0.lost and m0.N_lost == 1
    assert isinstance(m0.n_kept, int) and isinstance(m0.n_kept_local, int)
    assert not hasattr(pmetas[0][1], "fb_check") and not hasattr(pmetas[0][1], "n_kept")
    for _, m in metas[1:]:
        assert not hasattr(m, "fb_check") and isinstance(m.n_kept, int)
    # frame 0, both stages: the forward flow is the one of the run without the key (inside the template mask, all that run computes)
    inmask = cuda(seq["mask"].reshape(-1) > 0)
    assert len(log) >= 2 and len(plog) >= 2 and log[0]["judge"] and not log[1]["judge"]
    for k in (0, 1):
        a, b = log[k], plog[k]
        assert b["vis"] is None and a["vis"] is not None and a["vis"].numel() == HH * WW
        assert torch.equal(a["dst"][:, inmask].view(torch.int32), b["dst"][:, inmask].view(torch.int32)), k
        assert (a["w"] is None) == (b["w"] is None) == (raft_type == "orig")
        if a["w"] is not None:
            assert torch.equal(a["w"][:, inmask].view(torch.int32), b["w"][:, inmask].view(torch.int32)), k
        n_plain = int(ops.tc_flags(b["dst"] if b["bounds"] else None, b["tmask"], b["pw"], HH, WW, b["bounds"]).sum())
        print(f"{raft_type} stage {k}: {a['n_kept']} of {n_plain} template correspondences pass the check")
        assert 4 <= a["n_kept"] <= n_plain
    assert m0.n_kept == log[0]["n_kept"] and m0.n_kept_local == log[1]["n_kept"]
    # frame 0 by hand from the public pieces: compute_flow twice (and once in the correspondence form), fb_consistency, the gate
    prov = conf.flow_config.of_class(conf.flow_config)
    t, f0 = seq["template"], seq["frames"][0]
    tc = prov.compute_flow(t, f0, mode="TC", do_sigmoid=True)
    fwd = prov.compute_flow(t, f0, mode="flow")[0]
    bwd = prov.compute_flow(f0, t, mode="flow")[0]
    _, ok = fb_consistency(fwd, bwd, alpha=ALPHA, beta=BETA)
    for k in (0, 1):
        rec = log[k]
        assert torch.equal(rec["dst"].view(torch.int32), tc[1].view(torch.int32)) and torch.equal(rec["vis"].reshape(-1), ok.reshape(-1))
        if rec["w"] is not None:
            # (the tracker asks for the weights of the template mask's region only; elsewhere they are unspecified)
            assert torch.equal(rec["w"][:, inmask].view(torch.int32), tc[2][:, inmask].view(torch.int32))
        hand = dict(rec, dst=tc[1], w=tc[2], src=tc[0])
        Hm, n_kept = _fit_by_hand(conf, hand, ok.reshape(1, -1).contiguous(), device_backend)
        assert np.isfinite(Hm).all() and n_kept == rec["n_kept"] and np.array_equal(Hm, rec["H"]), (k, np.abs(Hm - rec["H"]).max())
    # every later solve: the recorded inputs through the same public pieces
    for k, rec in enumerate(log[2:], 2):
        assert set(np.unique(rec["vis"].cpu().numpy())) <= {0.0, 1.0}
        if rec["n_kept"] is not None and rec["n_kept"] >= 4 and rec["H"] is not None:
            Hm, n_kept = _fit_by_hand(conf, rec, rec["vis"], device_backend)
            assert n_kept == rec["n_kept"] and np.array_equal(Hm, rec["H"], equal_nan=True), k


def test_warm_start_carries_the_forward_flow_under_fb_check(seq, monkeypatch):
    """`warm_start_local` with `fb_check`: the flow carried to the next lost frame is the FORWARD one (the reverse flow is the
    provider's last call).  The frame t-1 -> t flow does not depend on the pose, so on a run of lost frames its correspondences
    are, frame by frame, those of the warm-started tracker without the key.  (The first lost frame's flow starts from the pinned
    template and runs in the other buffer set, so the second one starts cold too: the third and fourth are warm-started.)"""
    never = presets.redetection_by_inliers(1e-6, 0.999)
    local = {}
    for name, keys in (("fb", dict(fb_check="gate", fb_alpha=ALPHA, fb_beta=BETA)), ("plain", {})):
        trk, conf = _tracker(monkeypatch, "weighted", warm_start_local=True, redet_success_fn=never, **keys)
        log = _record_solves(trk)
        trk.init(seq["template"], seq["mask"])
        metas = [trk.track(f)[1] for f in seq["frames"] + [synth.make_frame(seq["template"], 4)]]
        assert [m.lost for m in metas] == [True] * 4 and [m.local_warm_started for m in metas] == [False, False, True, True], name
        local[name] = [r["dst"] for r in log if not r["judge"]]
    assert len(local["fb"]) == len(local["plain"]) == 4
    for i, (a, b) in enumerate(zip(local["fb"], local["plain"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i
