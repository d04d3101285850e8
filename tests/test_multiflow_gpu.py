"""The multi-delta chained tracker on the GPU: woft_flow_chain_fold against the float64 restatement
(tests/multiflow_host.py) on the same fp32 inputs -- selection, NaN and +inf patterns at every pixel, values within the 4 x
float32-yardstick rule with its 1e-6 floor -- ties, occlusion ordering, the null forms as bits, planted
non-finite values, a plane taller than one grid pass; MultiFlowTracker against chain_fold applied by hand to the provider's flows.

Measured on the MI355X (`pytest -s` prints them): (a) = the smallest cost margin, (b) = the smallest visibility margin of the
float64 restatement (multiflow_host.fold_all); then max |got - ref64| / its bound.

    case            (a)     (b)     flow              cost              vis
    5 x 7, K=1      -       0.2175  2.2e-07 / 3.5e-06 1.2e-08 / 1.0e-07 3.1e-08 / 9.4e-07
    9 x 70, K=3     0.4422  0.1603  3.7e-07 / 4.8e-06 6.9e-08 / 1.1e-06 1.1e-07 / 9.6e-07
    37 x 131, K=7   0.4355  0.1567  3.7e-07 / 4.8e-06 1.2e-07 / 3.1e-06 1.1e-07 / 9.6e-07
    262145 x 1, K=2 0.4241  0.1559  3.8e-07 / 5.0e-06 5.1e-08 / 6.2e-07 1.1e-07 / 9.6e-07
"""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multiflow_host as MH  # noqa: E402
from woft_amd import ops, synth  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
NAN, INF = float("nan"), float("inf")
THR = 0.5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_fold(best, prev, step, k, vis_thr=THR, unit_cost=1.0):
    """One woft_flow_chain_fold launch on numpy inputs; `best` = the device tuple of the folds so far (updated in place) or None."""
    prev = None if prev is None else tuple(cuda(p) for p in prev)
    return ops.flow_chain_fold(best, prev, cuda(step[0]), cuda(step[1]), cuda(step[2]), k=k, vis_thr=vis_thr, unit_cost=unit_cost,
                               first=best is None)


def gpu_fold_all(cands, order=None, **kw):
    best = None
    for k in (range(len(cands)) if order is None else order):
        best = gpu_fold(best, cands[k][0], cands[k][1], k, **kw)
    return host(best)


def host(best):
    return dict(zip(("flow", "cost", "vis", "sel"), (t.cpu().numpy() for t in best)))


def same_bits(a, b):
    return all(np.array_equal(bits(a[n]), bits(b[n])) for n in ("flow", "cost", "vis")) and np.array_equal(a["sel"], b["sel"])


def check_against_restatement(got, ref64, ref32, tag):
    """sel, the NaN pattern of flow and the +inf pattern of cost at EVERY pixel; on the finite pixels
    max |got - ref64| <= max(4 * max |ref32 - ref64|, 1e-6 * max |ref64|) for flow, cost and vis."""
    assert np.array_equal(got["sel"], ref64["sel"]), f"{tag}: {(got['sel'] != ref64['sel']).sum()} pixels select another candidate"
    assert np.array_equal(np.isnan(got["flow"]), np.isnan(ref64["flow"])) and np.array_equal(np.isposinf(got["cost"]), np.isposinf(ref64["cost"]))
    fin = ref64["sel"] >= 0
    assert np.array_equal(np.isnan(got["flow"][0]), ~fin) and np.array_equal(np.isposinf(got["cost"]), ~fin) and not got["vis"][~fin].any()
    report = []
    for n in ("flow", "cost", "vis"):
        r64, r32, g = ref64[n][..., fin], ref32[n][..., fin].astype(np.float64), got[n][..., fin].astype(np.float64)
        bound = max(4 * np.abs(r32 - r64).max(), 1e-6 * np.abs(r64).max())
        diff = np.abs(g - r64).max()
        report.append((n, diff, bound))
    print(f"{tag}: " + ", ".join(f"{n} {d:.1e} / {b:.1e}" for n, d, b in report))
    for n, diff, bound in report:
        assert diff <= bound, f"{tag}: {n} max |got - ref64| {diff:.3e} > {bound:.3e}"


# ---- 1. generated cases ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generated():
    """Per case: the candidates and the float64 / float32 restatements (computed once, left unchanged)."""
    out = {}
    for h, w, K in MH.CASES:
        cands = MH.make_case(h, w, K)
        ref64, margins = MH.fold_all(cands, THR)
        out[(h, w, K)] = dict(cands=cands, ref64=ref64, margins=margins, ref32=MH.fold_all(cands, THR, dtype=np.float32)[0])
    return out


@pytest.mark.parametrize("case", MH.CASES)
def test_generated_case_against_the_restatement(generated, case):
    c = generated[case]
    a, b = c["margins"]["cost"], c["margins"]["vis"]
    print(f"{case}: (a) smallest cost margin {a:.4f}, (b) smallest visibility margin {b:.4f}")
    assert a >= 1e-3 and b >= 1e-3
    check_against_restatement(gpu_fold_all(c["cands"]), c["ref64"], c["ref32"], f"{case}")


# ---- 2. ties --------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_earlier_fold(generated):
    prev, step = generated[(9, 70, 3)]["cands"][0]
    twins = [(prev, step), (prev, step)]
    for order in ((0, 1), (1, 0)):
        got = gpu_fold_all(twins, order)
        valid = got["sel"] >= 0
        assert valid.any() and (~valid).any() and (got["sel"][valid] == order[0]).all()
        assert same_bits(got, dict(gpu_fold_all(twins[:1]), sel=np.where(valid, order[0], -1).astype(np.int32)))


# ---- 3. occlusion ordering ------------------------------------------------------------------------------------------------------
def test_a_visible_candidate_beats_a_cheaper_occluded_one():
    h, w = 9, 70
    z, one = np.zeros((h, w), np.float32), np.ones((h, w), np.float32)
    flow = lambda v: np.stack([v * one, z]).astype(np.float32)
    # (no logits: cost = prev cost + unit cost 1, vis = prev vis, exactly)
    cheap_occluded = ((flow(0), 0.5 * one, 0.2 * one), (flow(1), None, None))
    dear_visible = ((flow(0), 3.0 * one, 0.9 * one), (flow(2), None, None))
    dearer_occluded = ((flow(0), 2.0 * one, 0.4 * one), (flow(3), None, None))
    for order in ((0, 1), (1, 0)):
        got = gpu_fold_all([cheap_occluded, dear_visible], order)
        assert (got["sel"] == 1).all() and (got["cost"] == 4.0).all() and (bits(got["vis"]) == bits(np.float32(0.9))).all()
        assert (got["flow"][0] == 2).all() and not got["flow"][1].any()
    for order in ((0, 1), (1, 0)):
        got = gpu_fold_all([cheap_occluded, dearer_occluded], order)
        assert (got["sel"] == 0).all() and (got["cost"] == 1.5).all() and (got["vis"] < THR).all() and (got["flow"][0] == 1).all()
    # the threshold is a strict one: vis == vis_thr is visible
    at_thr = ((flow(0), 9.0 * one, 0.5 * one), (flow(4), None, None))
    assert (gpu_fold_all([cheap_occluded, at_thr])["sel"] == 1).all()


# ---- 4. null forms, bit for bit -------------------------------------------------------------------------------------------------
def test_null_forms_as_bits(generated):
    cands = generated[(37, 131, 7)]["cands"]
    (pflow, pcost, pvis), (sflow, wl, ml) = cands[0]
    # null prev + first: q is the pixel itself, every pixel is valid, the flow planes are step_flow
    got = host(gpu_fold(None, None, (sflow, wl, ml), 5))
    assert (got["sel"] == 5).all() and np.array_equal(bits(got["flow"]), bits(sflow))
    r64 = np.log1p(np.exp(-wl.astype(np.float64)))                         # (the logits are 3 +- 0.3: no overflow to guard)
    r32 = MH.softplus_neg(wl).astype(np.float32).astype(np.float64)
    assert np.abs(got["cost"] - r64).max() <= max(4 * np.abs(r32 - r64).max(), 1e-6 * r64.max())
    v64 = 1 / (1 + np.exp(-ml.astype(np.float64)))
    v32 = (np.float32(1) / (np.float32(1) + np.exp(-ml))).astype(np.float64)
    assert np.abs(got["vis"] - v64).max() <= max(4 * np.abs(v32 - v64).max(), 1e-6 * v64.max())
    # null logits: cost = prev_cost + unit_cost, vis = prev_vis
    got = host(gpu_fold(None, (pflow, pcost, pvis), (sflow, None, None), 0, unit_cost=0.75))
    valid = got["sel"] >= 0
    assert valid.any() and (~valid).any()
    assert np.array_equal(bits(got["cost"][valid]), bits((pcost + np.float32(0.75))[valid]))
    assert np.array_equal(bits(got["vis"][valid]), bits(pvis[valid]))
    # a full prev with an all-zero step_wlogit: the flow of woft_flow_chain where valid, NaN where it is NaN
    got = host(gpu_fold(None, (pflow, pcost, pvis), (sflow, np.zeros_like(wl), ml), 0))
    chain = ops.flow_chain(cuda(pflow), cuda(sflow)).cpu().numpy()
    assert np.array_equal(np.isnan(chain[0]), got["sel"] < 0) and np.isnan(chain).any() and not np.isnan(chain).all()
    assert np.array_equal(bits(got["flow"]), bits(chain))                      # (NaN where it is NaN: the same quiet NaN)
    assert np.array_equal(np.isnan(got["flow"]), np.isnan(chain))


# ---- 5. non-finite inputs -------------------------------------------------------------------------------------------------------
PLANTED = dict(prev_flow=[((0, 2, 5), NAN), ((1, 3, 10), INF), ((0, 4, 15), -INF)],
               prev_cost=[((1, 20), NAN), ((2, 25), INF), ((3, 30), -INF)],
               step_flow=[((0, 4, 35), NAN), ((1, 5, 40), INF), ((0, 6, 45), -INF)],
               step_wlogit=[((1, 50), NAN), ((2, 55), INF), ((3, 60), -INF)],
               step_mlogit=[((5, 12), NAN), ((6, 22), INF), ((7, 32), -INF)])


def _plant(cand):
    """-> (the candidate with the values of PLANTED, the pixels it must be invalid at).  The affected pixels are found from the
    CLEAN fields only -- the pixel of a planted prev value, and every pixel one of whose four taps is a planted step pixel (a zero
    weight on an infinity is a NaN) -- no index is formed from a planted value."""
    (pflow, pcost, pvis), (sflow, wl, ml) = cand
    h, w = pcost.shape
    t = MH.taps(pflow)
    arrays = dict(prev_flow=pflow.copy(), prev_cost=pcost.copy(), step_flow=sflow.copy(), step_wlogit=wl.copy(), step_mlogit=ml.copy())
    affected = np.zeros((h, w), bool)
    for name, items in PLANTED.items():
        for idx, v in items:
            arrays[name][idx] = v
            y, x = idx[-2:]
            if name.startswith("prev"):
                affected[y, x] = True
            else:
                j = y * w + x
                affected |= t["valid"] & ((t["i00"] == j) | (t["i01"] == j) | (t["i10"] == j) | (t["i11"] == j))
    planted = ((arrays["prev_flow"], arrays["prev_cost"], pvis), (arrays["step_flow"], arrays["step_wlogit"], arrays["step_mlogit"]))
    return planted, affected


def test_planted_non_finite_values(generated):
    cands = generated[(9, 70, 3)]["cands"]
    # with `first`: the affected pixels are empty, every other pixel has the bits of the clean run
    planted, affected = _plant(cands[0])
    clean, got = gpu_fold_all(cands[:1]), gpu_fold_all([planted])
    assert affected.sum() >= 15 and (clean["sel"][affected] == 0).sum() >= 10
    assert (got["sel"][affected] == -1).all() and np.isnan(got["flow"][:, affected]).all()
    assert np.isposinf(got["cost"][affected]).all() and not got["vis"][affected].any()
    rest = ~affected
    assert all(np.array_equal(bits(got[n][..., rest]), bits(clean[n][..., rest])) for n in ("flow", "cost", "vis"))
    assert np.array_equal(got["sel"][rest], clean["sel"][rest])
    # folded second: the affected pixels keep the earlier best, every other pixel has the bits of the clean run
    planted, affected = _plant(cands[1])
    before, clean, got = gpu_fold_all(cands[:1]), gpu_fold_all(cands[:2]), gpu_fold_all([cands[0], planted])
    assert (clean["sel"][affected] == 1).sum() >= 3
    for n in ("flow", "cost", "vis"):
        assert np.array_equal(bits(got[n][..., affected]), bits(before[n][..., affected]))
        assert np.array_equal(bits(got[n][..., ~affected]), bits(clean[n][..., ~affected]))
    assert np.array_equal(got["sel"][affected], before["sel"][affected]) and np.array_equal(got["sel"][~affected], clean["sel"][~affected])
    assert np.array_equal(got["sel"], MH.fold_all([cands[0], planted], THR)[0]["sel"])


# ---- 6. a plane taller than one grid pass ---------------------------------------------------------------------------------------
def test_rows_beyond_one_grid_pass():
    h, w, K = 4 * 65535 + 5, 1, 2
    rs = np.random.RandomState(11)
    ys = np.arange(h, dtype=np.float64)[:, None]
    cands = []
    for k in range(K):
        col = lambda amp, lo=0.0: (lo + amp * np.sin(ys * rs.uniform(0.01, 0.02) + rs.uniform(0, 6))).astype(np.float32)
        zero = np.zeros((h, w), np.float32)
        pcost = (0.5 * ((np.arange(h)[:, None] // 3 + k) % K) + rs.uniform(0, 0.05, (h, w))).astype(np.float32)
        pvis = np.where(rs.uniform(size=(h, w)) < 0.3, rs.uniform(0.05, 0.3, (h, w)), rs.uniform(0.7, 1.0, (h, w))).astype(np.float32)
        cands.append(((np.stack([zero, col(3.0)]), pcost, pvis), (np.stack([zero, col(2.0)]), col(0.3, 3.0), col(0.3, 3.0))))
    ref64, m = MH.fold_all(cands, THR)
    ref32, _ = MH.fold_all(cands, THR, dtype=np.float32)
    assert m["cost"] >= 1e-3 and m["vis"] >= 1e-3
    tail = ref64["sel"][-5:]
    assert (ref64["sel"] == 0).any() and (ref64["sel"] == 1).any() and (ref64["sel"] < 0).any() and (tail >= 0).any()
    check_against_restatement(gpu_fold_all(cands), ref64, ref32, f"{h} x {w}")


# ---- 7. the tracker -------------------------------------------------------------------------------------------------------------
HH, WW, ITERS, N_FRAMES = 128, 160, 4, 6
MASK_HEAD = [(64, 3)]


@pytest.fixture(scope="module")
def frames():
    """A seeded random image shifted by integer offsets."""
    big = synth.make_template(HH + 32, WW + 32, seq_id=9)
    return [np.ascontiguousarray(big[16 - t:16 - t + HH, 16 + 2 * t:16 + 2 * t + WW]) for t in range(N_FRAMES)]


def _provider(raft_type, graph=False):
    from pytracking.utils.config import load_config
    fc = load_config(ROOT / "pytracking" / "optical_flow" / "configs" / "v2_SNOB_large_g05_RAFT.py")
    masked = raft_type == "weighted_masked"
    fc.model = synth.make_state_dict(seed=7, weighted=raft_type != "orig", mask_head_structure=MASK_HEAD if masked else None)
    fc.raft_type, fc.iters, fc.precision = raft_type, ITERS, "bf16x3"
    if masked:
        fc.class_params.mask_estimation, fc.class_params.mask_head_structure = True, MASK_HEAD
    if graph:
        fc.graph = True
    return fc.of_class(fc)


def _ibits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all(torch.equal(_ibits(getattr(a, n)), _ibits(getattr(b, n))) for n in ("flow", "cost", "vis", "occluded", "sel"))


def _run(trk, frames):
    trk.init(frames[0])
    return [trk.track(f) for f in frames[1:]]


@pytest.mark.parametrize("raft_type", ["orig", "weighted"])
def test_direct_candidate_alone_is_the_provider_flow(frames, raft_type):
    from woft_amd import MultiFlowTracker
    prov = _provider(raft_type)
    trk = MultiFlowTracker(prov, deltas=(None,))
    outs = _run(trk, frames[:3])
    assert trk._ring == {}
    for t, out in enumerate(outs, 1):
        flow, wts = prov.compute_flow(frames[0], frames[t], mode="flow")[:2]
        assert out.frame_index == t and [tuple(x.shape) for x in (out.flow, out.cost, out.vis, out.occluded, out.sel)] == \
            [(2, HH, WW)] + [(1, HH, WW)] * 4
        assert torch.equal(_ibits(out.flow), _ibits(flow)) and float(flow.abs().max()) > 0
        assert (out.sel == 0).all() and out.sel.dtype == torch.int32 and out.occluded.dtype == torch.bool
        assert (out.vis == 1).all() and not out.occluded.any()
        if raft_type == "orig":
            assert wts is None and (out.cost == 1).all()                   # (the unit cost)
        else:
            l = wts.cpu().numpy().astype(np.float64)
            r64 = np.log1p(np.exp(-np.abs(l))) + np.maximum(-l, 0)
            l32 = wts.cpu().numpy()
            r32 = MH.softplus_neg(l32).astype(np.float32).astype(np.float64)
            bound = max(4 * np.abs(r32 - r64).max(), 1e-6 * np.abs(r64).max())
            diff = np.abs(out.cost.cpu().numpy().astype(np.float64) - r64).max()
            print(f"frame {t}: cost max |got - ref64| {diff:.2e} / {bound:.2e}, logits in [{l.min():.2f}, {l.max():.2f}]")
            assert diff <= bound


@pytest.fixture(scope="module")
def eager_weighted():
    return {}


@pytest.mark.parametrize("deltas", [(None, 1, 2), (2, 1)])
@pytest.mark.parametrize("raft_type", ["orig", "weighted", "weighted_masked"])
def test_tracker_equals_chain_fold_by_hand(frames, raft_type, deltas, eager_weighted):
    """(None, 1, 2) is the issue's case; on seeded random weights its direct candidate is the cheapest everywhere, so (2, 1) --
    from frame 3 on two real chains compete -- is run as well."""
    from woft_amd import MultiFlowTracker, chain_fold
    prov = _provider(raft_type)
    trk = MultiFlowTracker(prov, deltas=deltas)
    trk.init(frames[0])
    z = lambda *s: torch.zeros(*s, device="cuda")
    stored = {0: (z(2, HH, WW), z(1, HH, WW), torch.ones(1, HH, WW, device="cuda"))}
    outs, wins = [], set()
    for t in range(1, N_FRAMES):
        out = trk.track(frames[t])
        keep = SimpleCopy(out)
        # by hand, with the provider's own (cloned) flows, in the same order; these calls also overwrite the provider's buffers
        best, exist = None, []
        for k, d in enumerate(deltas):
            s = 0 if d is None else t - d
            if s < 0:
                continue
            exist.append(k)
            res = prov.compute_flow(frames[s], frames[t], mode="flow")
            assert len(res) == (3 if raft_type == "weighted_masked" else 2) and (res[1] is None) == (raft_type == "orig")
            best = chain_fold(best, None if d is None else stored[s], tuple(res), k)
        stored[t] = best[:3]
        hand = SimpleCopy(None, flow=best[0], cost=best[1], vis=best[2], occluded=best[2] < 0.5, sel=best[3])
        assert _same(out, hand), (raft_type, t)
        assert _same(out, keep), "a further compute_flow changed the tracker's result"
        sel = set(torch.unique(out.sel).tolist())
        assert sel <= set(exist) | {-1} and sel & set(exist), (t, sel)
        wins |= sel
        assert sorted(trk._ring) == list(range(max(0, t - 1), t + 1))
        outs.append(keep)
    if deltas == (2, 1) and raft_type != "orig":           # (unit costs tie: the earlier fold takes every pixel both reach)
        assert {0, 1} <= wins, wins
    print(f"{raft_type} {deltas}: candidates that won somewhere: {sorted(wins)}; "
          f"{int((outs[-1].sel < 0).sum())} of {HH * WW} pixels without a valid chain at the last frame, "
          f"{int(outs[-1].occluded.sum())} occluded")
    # the ring owns its entries: none of them is a provider buffer
    own = {x.data_ptr() for o in prov._out.values() for x in o.values()}
    assert not own & {x.data_ptr() for img, r in trk._ring.values() for x in (img,) + tuple(r)}
    # reset, init and the same frames reproduce the bytes
    trk.reset()
    again = _run(trk, frames)
    assert len(again) == len(outs) and all(_same(a, b) for a, b in zip(again, outs))
    if raft_type == "weighted" and deltas == (None, 1, 2):
        eager_weighted["outs"] = outs


def test_graph_replay_gives_the_same_bytes(frames, eager_weighted):
    from woft_amd import MultiFlowTracker
    if "outs" not in eager_weighted:                       # (run alone: the eager results are computed here)
        eager_weighted["outs"] = _run(MultiFlowTracker(_provider("weighted"), deltas=(None, 1, 2)), frames)
    prov = _provider("weighted", graph=True)
    assert prov.use_graph
    outs = _run(MultiFlowTracker(prov, deltas=(None, 1, 2)), frames)
    assert all(_same(a, b) for a, b in zip(outs, eager_weighted["outs"])) and len(outs) == N_FRAMES - 1


def test_public_function_on_host_and_device_tensors(generated):
    """chain_fold: host tensors in, host tensors out, the bits of the device call; the caller's best is left alone."""
    from woft_amd import chain_fold
    cands = generated[(9, 70, 3)]["cands"]
    want = gpu_fold_all(cands)
    for dev in ("cpu", "cuda"):
        T = lambda a: torch.from_numpy(a).to(dev)
        best = None
        for k, (prev, step) in enumerate(cands):
            before = None if best is None else [b.clone() for b in best]
            new = chain_fold(best, tuple(T(p) for p in prev), tuple(T(s) for s in step), k)
            if before is not None:
                assert all(torch.equal(_ibits(a), _ibits(b)) for a, b in zip(best, before))
            best = new
        assert all(b.device.type == dev for b in best) and [tuple(b.shape) for b in best] == [(2, 9, 70)] + [(1, 9, 70)] * 3
        got = dict(zip(("flow", "cost", "vis", "sel"), (b.cpu().numpy().reshape(-1, 9, 70) for b in best)))
        assert np.array_equal(bits(got["flow"]), bits(want["flow"])) and np.array_equal(got["sel"][0], want["sel"])
        assert np.array_equal(bits(got["cost"][0]), bits(want["cost"])) and np.array_equal(bits(got["vis"][0]), bits(want["vis"]))


class SimpleCopy:
    """The fields of a track() result, cloned (or given)."""

    def __init__(self, out, **fields):
        for n in ("flow", "cost", "vis", "occluded", "sel"):
            setattr(self, n, fields[n] if out is None else getattr(out, n).clone())
