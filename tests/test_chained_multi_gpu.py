"""Several planar targets on one chained flow, on the GPU.  Every comparison is equality of bytes with the
existing single-target entry points or the existing tracker: woft_chain_tc_multi against K woft_chain_tc calls,
woft_tc_select_multi against K woft_tc_select_vis calls, woft_inlier_frac_batched against woft_inlier_frac, woft_hfit_batched
against ops.hfit(ws=...) (the equality the batched planar stage rests on), WOFTChainedMulti against K independent WOFTChained
trackers on a stub provider and on the real one, and the launches and device-to-host copies of a track(), which must not depend
on K."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import chained_multi_util as U  # noqa: E402
from launch_trace import d2h_copies  # noqa: E402
from woft_amd import _lib, ops, presets, synth  # noqa: E402
from woft_amd.chained import pack_target_bits  # noqa: E402

GRIDS = [(24, 40, None), (37, 53, (41, 60))]              # (gh, gw, mask size: None = the grid's); 37 x 53 has tail blocks


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tbits_of(masks):
    return cuda(pack_target_bits(masks).view(np.int32))


def u8(m):
    return cuda((np.asarray(m) != 0).astype(np.uint8) * 255)


# ---- 1. woft_chain_tc_multi -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("grid", GRIDS)
def test_chain_tc_multi_equals_k_single_calls(grid, K):
    gh, gw, mask_hw = grid
    mh, mw = mask_hw or (gh, gw)
    c = U.make_fold(gh, gw, seed=gh + K)
    masks = U.make_masks(mh, mw, K, seed=K)
    if K >= 3:
        assert not masks[1].any() and masks[2].all() and (masks[0] & masks[2]).any()
    dev = {k: cuda(v) for k, v in c.items()}
    tb = tbits_of(masks)
    for want_w in (True, False):
        dst, w, ok, hist = ops.chain_tc_multi(dev["flow"], dev["cost"], dev["vis"], dev["sel"], tb, K, 0.5, want_w=want_w,
                                              mask_hw=(mh, mw))
        again = ops.chain_tc_multi(dev["flow"], dev["cost"], dev["vis"], dev["sel"], tb, K, 0.5, want_w=want_w, mask_hw=(mh, mw))
        assert (w is None) == (not want_w) and tuple(hist.shape) == (K, ops.CHAIN_HIST)
        for a, b in zip((dst, w, ok, hist), again):                              # (two calls: equal bytes)
            assert a is None or torch.equal(a.view(torch.int32), b.view(torch.int32))
        for t in range(K):
            d1, w1, ok1, h1 = ops.chain_tc(dev["flow"], dev["cost"], dev["vis"], dev["sel"], u8(masks[t]), 0.5, want_w=want_w,
                                           mask_hw=(mh, mw))
            assert torch.equal(dst.view(torch.int32), d1.view(torch.int32)) and torch.equal(ok.view(torch.int32), ok1.view(torch.int32))
            assert w is None or torch.equal(w.view(torch.int32), w1.view(torch.int32))
            assert torch.equal(hist[t], h1), (t, hist[t].nonzero().flatten().tolist(), h1.nonzero().flatten().tolist())
            assert int(h1.sum()) == int((masks[t][:gh, :gw] != 0).sum())
    # the planted pixels reached the histograms: the full mask counts invalid and occluded pixels
    if K >= 3:
        assert int(hist[2, ops.CHAIN_HIST - 2]) >= 6 and int(hist[2, ops.CHAIN_HIST - 1]) > 0


# ---- 2. woft_tc_select_multi ------------------------------------------------------------------------------------------------------
def _select_inputs(gh, gw, seed):
    c = U.make_fold(gh, gw, seed=seed)
    dev = {k: cuda(v) for k, v in c.items()}
    full = torch.full((gh, gw), 255, dtype=torch.uint8, device="cuda")
    dst, w, ok, _ = ops.chain_tc(dev["flow"], dev["cost"], dev["vis"], dev["sel"], full, 0.5)
    assert bool(torch.isnan(dst).any()) and bool((dst < 0).any())               # (NaN and out-of-frame entries are in)
    return dst, w, ok, dev["vis"].reshape(1, -1).clone()


def _compare_select(dst, w, vis, vis_mode, vis_thr, masks, gh, gw, mh, mw, n_draw, cap):
    """One multi call against one woft_tc_select_vis call per target -> the (selected, kept) counts per target."""
    K, n = len(masks), gh * gw
    sobol = cuda(presets.sobol_points(n_draw).astype(np.float32)) if n_draw else None
    new = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")
    pa, pb, wo = new(K, cap, 2), new(K, cap, 2), new(K, cap)
    count = torch.full((2, K), -1, dtype=torch.int32, device="cuda")
    tb = tbits_of(masks)
    ops.tc_select_multi(dst, w, tb, K, mh, mw, True, sobol, vis, vis_mode, vis_thr, ops.tc_select_multi_ws(n, K), pa, pb, wo, count,
                        grid=(gh, gw))
    pa2, pb2, wo2, count2 = new(K, cap, 2), new(K, cap, 2), new(K, cap), torch.full((2, K), -1, dtype=torch.int32, device="cuda")
    ops.tc_select_multi(dst, w, tb, K, mh, mw, True, sobol, vis, vis_mode, vis_thr, ops.tc_select_multi_ws(n, K), pa2, pb2, wo2,
                        count2, grid=(gh, gw))
    got = count.cpu().numpy()
    assert np.array_equal(got, count2.cpu().numpy())
    ws1 = ops.tc_select_ws(n)
    for t in range(K):
        a1, b1, w1 = new(cap, 2), new(cap, 2), new(cap)
        c1 = torch.zeros(2, dtype=torch.int32, device="cuda")
        ops.tc_select_vis(dst, w, u8(masks[t]), None, mh, mw, True, sobol, vis, vis_mode, vis_thr, ws1, a1, b1, w1, c1, grid=(gh, gw))
        sel, kept = (int(v) for v in c1.cpu())
        assert (int(got[0, t]), int(got[1, t])) == (sel, kept), (t, got[:, t], sel, kept)
        for name, m, m2, s in (("pa", pa, pa2, a1), ("pb", pb, pb2, b1), ("w", wo, wo2, w1)):
            assert torch.equal(m[t, :sel].view(torch.int32), s[:sel].view(torch.int32)), (name, t, sel)
            assert torch.equal(m[t, :sel].view(torch.int32), m2[t, :sel].view(torch.int32)), (name, t)
    return got


SELECT_FORMS = [                                          # (n_draw, cap, weights, vis_mode)
    (100, 1024, True, "gate"), (100, 1024, False, "weight"), (100, 1024, True, None),
    (0, 50, True, "gate"), (0, 2000, True, "weight"), (0, 2000, False, "gate")]


@pytest.mark.parametrize("form", SELECT_FORMS)
@pytest.mark.parametrize("grid", GRIDS)
def test_tc_select_multi_equals_k_single_calls(grid, form):
    gh, gw, mask_hw = grid
    mh, mw = mask_hw or (gh, gw)
    n_draw, cap, weights, vis_mode = form
    dst, w, ok, vis = _select_inputs(gh, gw, seed=gh)
    masks = U.survivor_masks(mh, mw)
    # gate: the chains' 0 / 1 gate at 0.5, as the tracker passes it; weight: a probability; None: no visibility
    v = None if vis_mode is None else (ok if vis_mode == "gate" else vis)
    got = _compare_select(dst, w if weights else None, v, vis_mode, 0.5, masks, gh, gw, mh, mw, n_draw, cap)
    kept = got[1].tolist()
    assert kept[0] == 0 and 0 < kept[2] < 100 < kept[3]                         # none, fewer than n_draw, more than n_draw
    if n_draw:
        assert got[0, 2] == kept[2] and 0 < got[0, 3] <= n_draw                 # (keep-all below n_draw, a draw above it)
    else:
        assert got[0].tolist() == [min(k, cap) for k in kept] and (cap > kept[3]) == (cap == 2000)


def test_tc_select_multi_a_target_with_three_survivors():
    """Without a gate and with a flow that keeps the 1 x 3 mask inside the frame, exactly three correspondences survive."""
    gh, gw = 24, 40
    ys, xs = np.mgrid[:gh, :gw].astype(np.float32)
    dst = cuda(np.stack([xs + 0.25, ys - 0.5]).reshape(2, -1))
    dst[0, 10 * gw + 20], dst[1, 16 * gw + 30] = U.NAN, -3.0                     # (both inside the large mask alone)
    w = cuda(np.linspace(0.1, 1.0, gh * gw, dtype=np.float32)[None])
    got = _compare_select(dst, w, None, None, 0.5, U.survivor_masks(gh, gw), gh, gw, gh, gw, 100, 1024)
    assert got[1].tolist() == [0, 3, 48, 16 * 32 - 2] and got[0, 1] == 3


def test_tc_select_multi_uses_the_carry_above_1024_chunks():
    """1026 x 1024 pixels = 1026 chunks of 1024: select_plan scans the chunk counts 1024 at a time, the last two chunks' offsets
    need the carry.  One mask covers the frame, one only the last rows."""
    gh, gw = 1026, 1024
    rng = np.random.default_rng(5)
    ys, xs = np.mgrid[:gh, :gw].astype(np.float32)
    dst = np.stack([xs + rng.normal(0, 2, (gh, gw)).astype(np.float32), ys + rng.normal(0, 2, (gh, gw)).astype(np.float32)])
    dst[0, 100, 100] = U.NAN
    ok = (rng.uniform(0, 1, (gh, gw)) > 0.3).astype(np.float32)
    w = rng.uniform(0, 1, (1, gh * gw)).astype(np.float32)
    masks = [np.ones((gh, gw), np.uint8), np.zeros((gh, gw), np.uint8), np.zeros((gh, gw), np.uint8), np.zeros((gh, gw), np.uint8)]
    masks[1][1020:, 3:900] = 1
    masks[2][500:700, 200:600] = 1
    got = _compare_select(cuda(dst.reshape(2, -1)), cuda(w), cuda(ok.reshape(1, -1)), "gate", 0.5, masks, gh, gw, gh, gw, 500, 1024)
    assert got[1, 0] > 600000 and got[1, 1] > 2000 and got[1, 3] == 0 and 400 < got[0, 0] <= 500


# ---- 3. woft_inlier_frac_batched, woft_hfit_batched ---------------------------------------------------------------------------------
def _pairs(B, n, seed):
    rng = np.random.default_rng(seed)
    Ht = np.array([[1.02, 0.01, 3.0], [-0.02, 0.98, -2.0], [1e-5, -2e-5, 1.0]])
    pa = rng.uniform(0, 200, (B, n, 2))
    q = np.concatenate([pa, np.ones((B, n, 1))], 2) @ Ht.T
    pb = q[..., :2] / q[..., 2:] + rng.normal(0, 2.0, (B, n, 2))
    return cuda(pa.astype(np.float32)), cuda(pb.astype(np.float32)), Ht


@pytest.mark.parametrize("B", [1, 5])
def test_inlier_frac_batched_equals_singles(B):
    n_max = 300
    pa, pb, Ht = _pairs(B, n_max, seed=B)
    Hs = np.repeat(Ht[None], B, 0).astype(np.float32)
    Hs[B // 2] = U.NAN if B > 1 else Hs[0]                                       # (one NaN H)
    Hd = cuda(Hs.reshape(B, 9))
    counts = cuda(np.array([0, n_max, 7, n_max + 50, 123][:B] if B > 1 else [n_max], np.int32))
    for cnt in (counts, None):
        frac = torch.full((B,), -1.0, device="cuda")
        ops.inlier_frac_batched(pa, pb, Hd, frac, thr=2.5, counts=cnt)
        for b in range(B):
            f1 = torch.full((1,), -1.0, device="cuda")
            ops.inlier_frac(pa[b], pb[b], Hd[b], f1, thr=2.5, count=None if cnt is None else cnt[b:b + 1])
            assert torch.equal(frac[b:b + 1].view(torch.int32), f1.view(torch.int32)), (b, float(frac[b]), float(f1))
    assert 0.0 < float(frac[0]) < 1.0


@pytest.mark.parametrize("n", [500, 4])
def test_hfit_batched_has_the_bits_of_hfit_with_a_workspace(n):
    """The tracker's single-target stage calls ops.hfit(..., ws=fit_ws); up to 2048 correspondences that is the one-workgroup code
    woft_hfit_batched runs per element.  Weighted and IRLS, with counts."""
    B, cap = 3, 1024
    pa, pb, _ = _pairs(B, cap, seed=n)
    w = cuda(np.random.default_rng(n).uniform(0.05, 1.0, (B, cap)).astype(np.float32))
    counts = cuda(np.array([n, n, n], np.int32))
    ws = ops.hfit_ws("cuda")
    for reweight, k, n_irls in ((0, 0.0, 0), (2, 2.0, 5)):
        for wt in (w, None):
            Hb, sb = torch.zeros(B, 9, device="cuda"), torch.full((B,), -1, dtype=torch.int32, device="cuda")
            ops.hfit_batched(pa, pb, wt, Hb, sb, counts=counts, reweight=reweight, huber_k=k, n_irls=n_irls)
            for b in range(B):
                H1, s1 = torch.zeros(9, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda")
                ops.hfit(pa[b], pb[b], None if wt is None else wt[b], H1, s1, count=counts[b:b + 1], reweight=reweight, huber_k=k,
                         n_irls=n_irls, ws=ws)
                assert int(s1) == int(sb[b]) and (n == 4 or int(s1) == 0)
                assert torch.equal(Hb[b].view(torch.int32), H1.view(torch.int32)), (n, reweight, b)


# ---- 4. the tracker on a stub provider ----------------------------------------------------------------------------------------------
def _run_stub(monkeypatch, fused=True, **kw):
    """-> (multi tracker, its results per frame, per target the results of an independent WOFTChained)."""
    monkeypatch.setenv("WOFT_FUSED", "1" if fused else "0")
    frame0, frames = U.stub_frames()
    masks = U.stub_masks()
    conf = U.stub_config(True, **kw)
    trk = conf.tracker_class(conf)
    trk.init(frame0, masks)
    multi = [trk.track(f) for f in frames]
    singles = []
    for m in masks:
        c1 = U.stub_config(False, **kw)
        one = c1.tracker_class(c1)
        one.init(frame0, m)
        singles.append([one.track(f) for f in frames])
    return trk, multi, singles


def _check_stub(trk, multi, singles, tag):
    U.assert_same_result(multi, singles, tag)
    for f, (Hs, metas) in enumerate(multi, 1):
        # the 1 x 3 target never has 4 correspondences: lost, its previous (initial) pose kept; the others are tracked
        assert metas[2].lost and metas[2].N_lost == f and metas[2].n_kept <= 3 and np.array_equal(Hs[2], np.eye(3))
        assert metas[2].H_global_cur2init is None
        assert not metas[0].lost and not metas[1].lost and not np.array_equal(Hs[0], np.eye(3))
        assert hasattr(metas[0], "solver_decision") == (f == 1) == hasattr(metas[2], "precision")
    assert "multi-target planar stage" in trk.solver_decision and "multi-target" not in multi[0][1][0].solver_decision


@pytest.mark.parametrize("raft_type,occlude", [("weighted", None), ("orig", None), ("weighted_masked", "left@3")])
def test_stub_tracker_equals_independent_trackers(monkeypatch, raft_type, occlude):
    trk, multi, singles = _run_stub(monkeypatch, raft_type=raft_type, occlude=occlude)
    assert trk._route == "batched" and "one batched fit" in trk.solver_decision
    _check_stub(trk, multi, singles, raft_type)
    if occlude:
        assert multi[2][1][0].chain_occluded > 0 and multi[1][1][0].chain_occluded == 0
    # one dense track for all targets: the provider was asked for one schedule's flows per frame
    assert trk.flower.n_calls == sum(len(trk.multi.schedule(t)) for t in range(1, U.S_FRAMES + 1))


def test_stub_tracker_ransac_preset(monkeypatch):
    trk, multi, singles = _run_stub(monkeypatch, estimator=presets.estimator_ransac(10000, 3.0, 0.995))
    assert trk._route == "select" and "RANSAC" in trk.solver_decision
    _check_stub(trk, multi, singles, "ransac")


def test_stub_tracker_callable_back_end(monkeypatch):
    trk, multi, singles = _run_stub(monkeypatch, fused=False)
    assert trk._fused is None and trk._route == "loop" and "loop" in trk.solver_decision
    _check_stub(trk, multi, singles, "callables")


def test_stub_tracker_masks_as_an_array_and_reinit(monkeypatch):
    """(K, H, W) bool array in, and init() again starts every target over."""
    monkeypatch.setenv("WOFT_FUSED", "1")
    frame0, frames = U.stub_frames()
    conf = U.stub_config(True)
    trk = conf.tracker_class(conf)
    trk.init(frame0, U.stub_masks())
    first = [trk.track(f) for f in frames[:2]]
    trk.init(frame0, np.stack(U.stub_masks()) > 0)
    again = [trk.track(f) for f in frames[:2]]
    for (Ha, ma), (Hb, mb) in zip(first, again):
        assert np.array_equal(Ha, Hb) and [m.N_lost for m in ma] == [m.N_lost for m in mb]
    assert not hasattr(again[0][1][0], "solver_decision")                        # (announced once per tracker, as the parent)


# ---- 5. the tracker on the real provider --------------------------------------------------------------------------------------------
def _real_config(multi, padding_mode):
    from pytracking.utils.config import load_config
    conf = load_config(U.ROOT / "pytracking" / "configs" / ("WOFT_chained_multi.py" if multi else "WOFT_chained.py"))
    fc = conf.flow_config
    fc.model = synth.make_state_dict(seed=7, weighted=True)
    fc.raft_type, fc.iters, fc.precision = "weighted", 4, "bf16x3"
    if padding_mode:
        fc.padding_mode = padding_mode
    conf.chain_deltas = (None, 1)
    return conf


@pytest.mark.parametrize("padding_mode,hw", [(None, (128, 160)), ("crop", (131, 163))])
def test_real_provider_equals_independent_trackers(padding_mode, hw):
    Hh, Ww = hw
    template = synth.make_template(Hh, Ww, seq_id=3)
    frames = [synth.make_frame(template, t) for t in (1, 2, 3)]
    a = synth.make_init_mask(Hh, Ww)
    b = np.zeros_like(a)
    b[Hh // 8:Hh // 2, Ww // 4:3 * Ww // 4] = 255
    masks = [a, b]
    assert ((a > 0) & (b > 0)).any()
    conf = _real_config(True, padding_mode)
    trk = conf.tracker_class(conf)
    assert trk._route == "batched" and trk._fused["n_draw"] == 500
    trk.init(template, masks)
    multi = [trk.track(f) for f in frames]
    singles = []
    for m in masks:
        c1 = _real_config(False, padding_mode)
        one = c1.tracker_class(c1)
        one.init(template, m)
        singles.append([one.track(f) for f in frames])
    U.assert_same_result(multi, singles, str(padding_mode))
    assert any(m.n_kept >= 4 and m.H_global_cur2init is not None for _, metas in multi for m in metas)


# ---- 6. launches and reads do not depend on K ---------------------------------------------------------------------------------------
def _trace_one_track(monkeypatch, K):
    """-> (the entry points one preset-path track() calls, its device-to-host copies)."""
    monkeypatch.setenv("WOFT_FUSED", "1")
    frame0, frames = U.stub_frames()
    masks = []
    for t in range(K):
        m = np.zeros((U.SH, U.SW), np.uint8)
        m[4 + t:30 + t, 6 + 2 * t:40 + 2 * t] = 255
        masks.append(m)
    conf = U.stub_config(True)
    trk = conf.tracker_class(conf)
    trk.init(frame0, masks)
    trk.track(frames[0])                                                         # (buffers allocated, library loaded)
    copies = []
    with pytest.MonkeyPatch.context() as patch:
        proxy = U.CountingLib(_lib.load())
        patch.setattr(_lib, "_lib", proxy)
        d2h_copies(patch, copies.append)
        Hs, metas = trk.track(frames[1])
        torch.cuda.synchronize()
    assert Hs.shape == (K, 3, 3) and not any(m.lost for m in metas)
    return proxy.calls, copies


def test_launches_and_reads_do_not_depend_on_k(monkeypatch):
    calls1, copies1 = _trace_one_track(monkeypatch, 1)
    calls8, copies8 = _trace_one_track(monkeypatch, 8)
    assert calls1 == calls8, (calls1, calls8)
    planar = [c for c in calls1 if c != "woft_flow_chain_fold"]
    assert planar == ["woft_chain_tc_multi", "woft_tc_select_multi", "woft_hfit_batched", "woft_inlier_frac_batched"], planar
    assert copies1 == copies8 == ["copy_"], (copies1, copies8)
