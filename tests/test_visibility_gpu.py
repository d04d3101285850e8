"""The tracker's visibility modes on the GPU (DESIGN.md "Visibility mask in the tracker").

Kernels: `woft_tc_select_vis` / `woft_tc_flags_vis` against the numpy restatement (tests/visibility_host.py), bit for bit -- the two
rules have no transcendental and no reduction --, and against `woft_tc_select` where no visibility is given.
Tracker: both modes, both solver back ends and a host replay (the provider's own outputs -> visibility_host -> ops.hfit) return the
same bits; WOFTWindow; and a 'weighted' config without a mode never reaches the new entry points."""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_refs as R  # noqa: E402
import visibility_host as V  # noqa: E402
from woft_amd import ops, presets, synth  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
THR = 0.5
NAN = float("nan")
PLANTED = [THR, 0.0, 1.0, NAN]


# ---- kernels --------------------------------------------------------------------------------------------------------------------
# (gh, gw, mh, mw, share of the template mask): 960 grid pixels at 45 % leave fewer than 500 survivors in either mode, and 9 100
# pixels (nine 1024-pixel workgroups, whose counts the plan kernel scans) at 4.5 % as well; more than 64 survive every case.
_GEO = {"same": (24, 40, 24, 40, 0.45), "crop": (24, 40, 27, 45, 0.45), "blocks": (70, 130, 70, 130, 0.045)}


def _case(name):
    gh, gw, mh, mw, dens = _GEO[name]
    rs = np.random.RandomState({"same": 11, "crop": 12, "blocks": 13}[name])
    n = gh * gw
    i = np.arange(n)
    dst = np.stack([rs.uniform(-2, mw + 2, n), rs.uniform(-2, mh + 2, n)]).astype(np.float32)
    tmask = ((rs.uniform(size=(mh, mw)) < dens) * 255).astype(np.uint8)
    pw = (rs.uniform(size=(mh, mw)) < 0.9).astype(np.uint8)
    vis = rs.uniform(0, 1, n).astype(np.float32)
    w = rs.uniform(0.05, 1, n).astype(np.float32)
    # planted visibilities: exactly thr, 0, 1 and NaN -- on the first and last grid pixel, inside and outside the template mask
    inside = np.flatnonzero(tmask[i // gw, i % gw] != 0)
    outside = np.flatnonzero(tmask[i // gw, i % gw] == 0)
    inside, outside = inside[(inside > 0) & (inside < n - 1)], outside[(outside > 0) & (outside < n - 1)]
    spots = np.concatenate([[0, n - 1], rs.choice(inside, 8, replace=False), rs.choice(outside, 4, replace=False)])
    vals = [THR, NAN] + PLANTED + PLANTED + PLANTED
    tmask[0, 0] = tmask[(n - 1) // gw, (n - 1) % gw] = 255
    for s, v in zip(spots, vals):
        vis[s] = v
        y, x = s // gw, s % gw
        dst[:, s] = (x, y)                       # in bounds, on a pre-warp pixel that is set: the visibility alone decides
        pw[y, x] = 1
    return dict(gh=gh, gw=gw, mh=mh, mw=mw, dst=dst, tmask=tmask, pw=pw, vis=vis, w=w, spots=spots)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_select(c, dev, check_dst, pw, u, w, vis, mode, thr, cap, plain=False):
    n = c["gh"] * c["gw"]
    pa = torch.full((cap + 16, 2), 1e30, device="cuda")
    pb = torch.full((cap + 16, 2), 1e30, device="cuda")
    wo = torch.full((cap + 16,), 1e30, device="cuda")
    cnt = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    ws = ops.tc_select_ws(n)
    args = (dev["dst"], dev["w"] if w else None, dev["tmask"], dev["pw"] if pw else None, c["mh"], c["mw"], check_dst, _cuda(u))
    if plain:
        ops.tc_select(*args, ws, pa[:cap], pb[:cap], wo[:cap], cnt, grid=(c["gh"], c["gw"]))
    else:
        ops.tc_select_vis(*args, dev["vis"] if vis else None, mode, thr, ws, pa[:cap], pb[:cap], wo[:cap], cnt,
                          grid=(c["gh"], c["gw"]))
    torch.cuda.synchronize()
    return pa.cpu().numpy(), pb.cpu().numpy(), wo.cpu().numpy(), cnt.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in _GEO:
        c = _case(name)
        out[name] = (c, {k: _cuda(c[k]) for k in ("dst", "tmask", "pw", "vis", "w")})
    return out


@pytest.mark.parametrize("mode", [V.GATE, V.WEIGHT])
@pytest.mark.parametrize("name", list(_GEO))
def test_select_vis_bit_for_bit_against_numpy(cases, name, mode):
    c, dev = cases[name]
    gh, gw = c["gh"], c["gw"]
    n = gh * gw
    for check_dst in (0, 1):
        for pw in (False, True):
            for n_draw in (0, 500, 64):
                u = presets.sobol_points(n_draw).astype(np.float32) if n_draw else None
                cap = 1024 if n_draw else n
                for use_w in (True, False):
                    ref = V.select_vis(c["dst"], c["w"] if use_w else None, c["tmask"], c["pw"] if pw else None, gh, gw,
                                       np.zeros(0, np.float32) if u is None else u, cap, c["vis"], mode, THR, check_dst=bool(check_dst))
                    rpa, rpb, rwo, m, nk = ref
                    # the cases are what they are meant to be: a 500-draw on fewer than 500 survivors, a 64-draw on more than 64
                    assert 64 < nk < 500, (name, mode, check_dst, pw, nk)
                    assert m == (nk if n_draw in (0, 500) else len(np.unique(np.rint(np.float32(nk) * u))))
                    pa, pb, wo, cnt = _run_select(c, dev, check_dst, pw, u, use_w, True, mode, THR, cap)
                    tag = (name, mode, check_dst, pw, n_draw, use_w)
                    assert (int(cnt[0]), int(cnt[1])) == (m, nk), tag
                    assert np.array_equal(pa[:m].view(np.uint32), np.ascontiguousarray(rpa).view(np.uint32)), tag      # (bits: NaN targets included)
                    assert np.array_equal(pb[:m], rpb), tag
                    assert np.array_equal(wo[:m].view(np.uint32), rwo.view(np.uint32)), tag
                    for t in (pa, pb, wo):
                        assert (t[m:] == np.float32(1e30)).all(), tag                          # nothing written past the count
    # the planted values did what they are there for: thr, 0 and NaN are gated away, 1 stays (first / last pixel included)
    keep = V.keep_rule_vis(c["dst"], c["tmask"], c["pw"], gh, gw, c["vis"], V.GATE, THR)
    plain = R.keep_rule(c["dst"], c["tmask"], c["pw"], gh, gw)
    sp = c["spots"]
    assert plain[0] and plain[n - 1] and not keep[0] and not keep[n - 1]
    assert plain[sp[2:10]].all() and list(keep[sp[2:10]]) == [False, False, True, False] * 2
    assert not plain[sp[10:14]].any() and not keep[sp[10:14]].any()


@pytest.mark.parametrize("name", list(_GEO))
def test_without_visibility_select_vis_is_select(cases, name):
    """vis = NULL (any mode) and vis_mode = 0 (any vis): the outputs of woft_tc_select on the same inputs, every slot."""
    c, dev = cases[name]
    n = c["gh"] * c["gw"]
    for check_dst, pw, n_draw, use_w in ((1, True, 64, True), (1, False, 0, False), (0, False, 500, True), (0, True, 64, False)):
        u = presets.sobol_points(n_draw).astype(np.float32) if n_draw else None
        cap = 1024 if n_draw else n
        want = _run_select(c, dev, check_dst, pw, u, use_w, False, 0, 0.0, cap, plain=True)
        for vis, mode, thr in ((False, V.GATE, THR), (False, V.WEIGHT, THR), (True, 0, THR), (True, None, 0.0)):
            got = _run_select(c, dev, check_dst, pw, u, use_w, vis, mode, thr, cap)
            for a, b in zip(got, want):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, check_dst, pw, n_draw, use_w, vis, mode)


@pytest.mark.parametrize("name", list(_GEO))
def test_flags_vis_agrees_with_the_select_kernel(cases, name):
    c, dev = cases[name]
    gh, gw, mh, mw = c["gh"], c["gw"], c["mh"], c["mw"]
    n = gh * gw
    for check_dst in (0, 1):
        for pw in (False, True):
            pwd, pwh = (dev["pw"], c["pw"]) if pw else (None, None)
            for mode in (V.GATE, V.WEIGHT, 0):
                flags = ops.tc_flags_vis(dev["dst"] if check_dst else None, dev["tmask"], pwd, mh, mw, check_dst, dev["vis"], mode, THR,
                                         grid=(gh, gw))
                torch.cuda.synchronize()
                flags = flags.cpu().numpy()
                assert np.array_equal(flags, V.keep_rule_vis(c["dst"], c["tmask"], pwh, gh, gw, c["vis"], mode, THR,
                                                             check_dst=bool(check_dst)))
                # what the select kernel kept (no draw, room for everything): the source pixels in pb
                _, pb, _, cnt = _run_select(c, dev, check_dst, pw, None, True, True, mode, THR, n)
                implied = np.zeros(n, bool)
                k = int(cnt[0])
                implied[(pb[:k, 1] * gw + pb[:k, 0]).astype(np.int64)] = True
                assert k == int(cnt[1]) == int(flags.sum()) and np.array_equal(implied, flags), (name, check_dst, pw, mode)
            plain = ops.tc_flags(dev["dst"] if check_dst else None, dev["tmask"], pwd, mh, mw, check_dst, grid=(gh, gw))
            none = ops.tc_flags_vis(dev["dst"] if check_dst else None, dev["tmask"], pwd, mh, mw, check_dst, None, V.GATE, THR,
                                    grid=(gh, gw))
            assert torch.equal(plain, none)


# ---- tracker --------------------------------------------------------------------------------------------------------------------
HH, WW, ITERS, STRUCTURE = 128, 160, 4, [(128, 3), (128, 3)]
TS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def seq():
    sd = synth.make_state_dict(seed=7, mask_head_structure=STRUCTURE)
    template = synth.make_template(HH, WW, seq_id=5)
    return dict(sd=sd, template=template, mask=synth.make_init_mask(HH, WW), frames=[synth.make_frame(template, t) for t in TS])


def _tracker(seq, monkeypatch, backend, cfg="WOFT_visibility.py", padding_mode=None, **keys):
    from pytracking.utils.config import load_config
    monkeypatch.setenv("WOFT_FUSED", "1")
    conf = load_config(ROOT / "pytracking" / "configs" / cfg)
    conf.flow_config.model = seq["sd"]
    conf.flow_config.iters = ITERS
    conf.flow_config.precision = "fp32"
    if padding_mode:
        conf.flow_config.padding_mode = padding_mode
    if backend == "callables":
        conf.device_solver = False
    for k, v in keys.items():
        setattr(conf, k, v)
    trk = conf.tracker_class(conf)
    assert (trk._fused is not None) == (backend == "device")
    return trk


@pytest.fixture(scope="module")
def median_thr(seq):
    """Seeded random weights give an arbitrary mask: the gate's threshold is the median visibility of the template pixels in one
    flow (the provider's own output under the tracker's request), so that the gate neither keeps everything nor nothing."""
    mp = pytest.MonkeyPatch()
    try:
        trk = _tracker(seq, mp, "device")
        out = trk.flower.compute_flow(seq["template"], seq["frames"][0], mode="TC", do_sigmoid=True, visibility=True)
        logits = trk.flower.compute_flow(seq["template"], seq["frames"][0], mode="TC", do_sigmoid=True)[3]
    finally:
        mp.undo()
    p = out[3].cpu().numpy().reshape(-1)
    assert p.shape == (HH * WW,) and np.all((p >= 0) & (p <= 1))
    # the request changes the fourth value only: the probability of the logits every other caller gets (fp32 expf and a division
    # on values in [0, 1]: a few ulp of 1, 1e-6)
    assert torch.allclose(out[3], torch.sigmoid(logits), atol=1e-6) and float(logits.abs().max()) > 0
    thr = float(np.float32(np.median(p[seq["mask"].reshape(-1) > 0])))
    print(f"median visibility of the template pixels: {thr:.6f} (p in [{p.min():.4f}, {p.max():.4f}])")
    assert 0.0 < thr < 1.0 and p.max() < 0.999999
    return thr


def _record_solves(trk):
    """Wrap the instance's _solve: keep the provider's outputs and the masks of every solve, with the fit it returned."""
    log, inner = [], trk._solve

    def solve(src_xy, dst_xy, w, grid, frame_hw, src_mask_u8, dst_valid_u8, bounds, judge, vis=None):
        rec = dict(dst=dst_xy.cpu().numpy().copy(), w=None if w is None else w.cpu().numpy().copy(), vis=None if vis is None else vis.cpu().numpy().copy(),
                   grid=grid, frame_hw=tuple(frame_hw), tmask=src_mask_u8.cpu().numpy().copy(),
                   pw=None if dst_valid_u8 is None else dst_valid_u8.cpu().numpy().copy(), bounds=bounds, judge=judge, H=None)
        log.append(rec)
        fit = inner(src_xy, dst_xy, w, grid, frame_hw, src_mask_u8, dst_valid_u8, bounds, judge, vis=vis)
        rec["H"], rec["n_kept"] = fit.H.copy(), trk.n_kept
        return fit
    trk._solve = solve
    return log


def _replay(rec, mode, thr, u):
    """One recorded solve on the host: visibility_host on the provider's outputs, then ops.hfit on the selected set."""
    Hh, Ww = rec["frame_hw"]
    gh, gw = rec["grid"] or (Hh, Ww)
    pa, pb, wo, m, nk = V.select_vis(rec["dst"], rec["w"], rec["tmask"].reshape(Hh, Ww), rec["pw"], gh, gw, u, 1024, rec["vis"], mode,
                                     thr, check_dst=bool(rec["bounds"]))
    n_plain = int(R.keep_rule(rec["dst"], rec["tmask"].reshape(Hh, Ww), rec["pw"], gh, gw, check_dst=bool(rec["bounds"])).sum())
    Hout = torch.empty(9, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.hfit(_cuda(pa), _cuda(pb), _cuda(wo), Hout, status)
    torch.cuda.synchronize()
    return Hout.cpu().numpy().astype(np.float64).reshape(3, 3), int(status[0]), nk, n_plain


@pytest.mark.parametrize("mode", [V.GATE, V.WEIGHT])
def test_tracker_back_ends_and_host_replay_are_bit_identical(seq, median_thr, monkeypatch, mode):
    u = presets.sobol_points(500).astype(np.float32)
    runs = {}
    for backend in ("device", "callables"):
        trk = _tracker(seq, monkeypatch, backend, visibility_mode=mode, visibility_thr=median_thr)
        assert f"visibility {mode}" in trk.solver_decision and trk.visibility_thr == median_thr
        log = _record_solves(trk)
        trk.init(seq["template"], seq["mask"])
        out = []
        for i, f in enumerate(seq["frames"]):
            Hc, meta = trk.track(f)
            out.append((Hc, meta))
            assert (meta.visibility_mode == mode and meta.solver_decision == trk.solver_decision) if i == 0 \
                else not hasattr(meta, "visibility_mode")
        runs[backend] = (out, log)
    (da, la), (db, lb) = runs["device"], runs["callables"]
    assert len(la) == len(lb) >= len(TS)
    for i, ((Ha, ma), (Hb, mb)) in enumerate(zip(da, db)):
        assert np.array_equal(Ha, Hb), (i, np.abs(Ha - Hb).max())
        assert ma.n_kept == mb.n_kept and ma.lost == mb.lost and bool(ma.global_H_success) == bool(mb.global_H_success)
        assert getattr(ma, "n_kept_local", None) == getattr(mb, "n_kept_local", None)
        assert np.array_equal(ma.H_global_cur2init, mb.H_global_cur2init)
    n_in_mask = int((seq["mask"] > 0).sum())
    for k, (ra, rb) in enumerate(zip(la, lb)):
        assert np.array_equal(ra["dst"].view(np.uint32), rb["dst"].view(np.uint32)) and np.array_equal(ra["vis"], rb["vis"])
        Hr, status, nk, n_plain = _replay(ra, mode, median_thr, u)
        print(f"{mode} solve {k} ({'global' if ra['judge'] else 'local'}): {nk} of {n_plain} template correspondences survive")
        assert status == 0 and ra["n_kept"] == rb["n_kept"] == nk
        assert np.array_equal(ra["H"], Hr) and np.array_equal(rb["H"], Hr), (k, np.abs(ra["H"] - Hr).max())
        if mode == V.GATE:          # conditions of the test: the gate keeps neither everything nor nothing
            assert 4 <= nk < n_plain <= n_in_mask, (k, nk, n_plain)
        else:
            assert nk == n_plain
    globals_ = [r for r in la if r["judge"]]
    assert [m.n_kept for _, m in da] == [r["n_kept"] for r in globals_]


@pytest.mark.parametrize("backend", ["device", "callables"])
def test_gate_that_leaves_fewer_than_four_reports_the_frame_lost(seq, median_thr, monkeypatch, backend):
    trk = _tracker(seq, monkeypatch, backend, visibility_mode="gate", visibility_thr=0.999999)
    trk.init(seq["template"], seq["mask"])
    Hc, meta = trk.track(seq["frames"][0])
    assert meta.n_kept < 4 and meta.lost and not meta.global_H_success and meta.N_lost == 1
    assert np.array_equal(Hc, np.eye(3)) and np.array_equal(meta.H_local_cur2init, np.eye(3))     # the previous pose is kept
    assert meta.n_kept_local < 4


def test_window_tracker_in_gate_mode(seq, median_thr, monkeypatch):
    from pytracking.tracker.WOFT_window import WOFTWindow
    runs = []
    for backend in ("device", "callables"):
        trk = _tracker(seq, monkeypatch, backend, padding_mode="RAFT", tracker_class=WOFTWindow, search_window_margin=0.25,
                       visibility_mode="gate", visibility_thr=median_thr)
        assert type(trk) is WOFTWindow
        trk.init(seq["template"], seq["mask"])
        rows, cols = trk._rect[2], trk._rect[3]
        assert (rows, cols) != (HH, WW)                                    # the mask is on the window's grid, not the frame's
        out = []
        for f in seq["frames"][:3]:
            Hc, meta = trk.track(f)
            out.append((Hc, meta, trk.local_search_bbox))
        runs.append(out)
    for (Ha, ma, ba), (Hb, mb, bb) in zip(*runs):
        assert np.array_equal(Ha, Hb) and ma.n_kept == mb.n_kept and ma.lost == mb.lost and ba == bb
        assert 4 <= ma.n_kept < rows * cols
        assert getattr(ma, "n_kept_local", None) == getattr(mb, "n_kept_local", None)


def test_without_a_mode_a_weighted_config_is_as_before(seq, monkeypatch):
    """visibility_mode absent / None: the same H as YAOFTrackerSingleControl's host replay of the plain rule, and the new entry
    points are never reached."""
    def never(*a, **k):
        raise AssertionError("a 'weighted' config reached a visibility entry point")
    monkeypatch.setattr(ops, "tc_select_vis", never)
    monkeypatch.setattr(ops, "tc_flags_vis", never)
    u = presets.sobol_points(500).astype(np.float32)
    plain = dict(seq, sd=synth.make_state_dict(seed=7))
    for k, v in plain["sd"].items():                                       # (the mask head is drawn last: the same network without it)
        assert torch.equal(v, seq["sd"][k])
    results = []
    for backend, keys in (("device", {}), ("device", dict(visibility_mode=None)), ("callables", {})):
        trk = _tracker(plain, monkeypatch, backend, cfg="WOFT.py", **keys)
        assert trk.visibility_mode is None and "visibility" not in trk.solver_decision
        log = _record_solves(trk)
        trk.init(seq["template"], seq["mask"])
        out = []
        for f in seq["frames"]:
            Hc, meta = trk.track(f)
            assert not hasattr(meta, "n_kept") and not hasattr(meta, "visibility_mode")
            out.append(Hc)
        results.append(out)
        for rec in log:
            assert rec["vis"] is None
            Hr, status, nk, n_plain = _replay(rec, None, 0.0, u)
            assert status == 0 and nk == n_plain and np.array_equal(rec["H"], Hr)
    for other in results[1:]:
        for Ha, Hb in zip(results[0], other):
            assert np.array_equal(Ha, Hb)
