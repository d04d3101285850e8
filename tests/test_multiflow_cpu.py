"""The multi-delta chained tracker on the host: the new entry point in the header, EXPORTS and the library,
its argument checks (-1 before any device work), every construction error of MultiFlowTracker, the delta schedule and the ring's
eviction (a fake provider and a fake fold: nothing is computed), and the numpy restatement of the fold against values worked out
by hand."""
import ctypes
import math
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import multiflow_host as MH

ROOT = Path(__file__).resolve().parent.parent
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_exports_and_library_agree_on_the_new_name(lib):
    from woft_amd import _lib
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    name = "woft_flow_chain_fold"
    assert name in declared and name in _lib.EXPORTS and hasattr(raw, name)
    assert len(_lib._SIGS[name][1]) == 17
    assert lib.woft_abi_version() == raw.woft_abi_version()


def test_fold_rejects_bad_arguments_without_a_device(lib):
    """-1 before any launch (host buffers stand in for device ones: nothing is dereferenced).  Every plane of the base call is a
    buffer of its own, so each case has exactly one thing wrong."""
    h, w = 5, 7
    buf = (ctypes.c_float * 8192)()
    base = ctypes.addressof(buf)
    at = lambda j: base + 4 * 512 * j                         # (2 KiB apart: a 5 x 7 flow is 280 B)
    good = dict(prev_flow=at(0), prev_cost=at(1), prev_vis=at(2), step_flow=at(3), step_wlogit=at(4), step_mlogit=at(5), h=h, w=w,
                unit_cost=1.0, vis_thr=0.5, k=3, first=0, best_flow=at(6), best_cost=at(7), best_vis=at(8), best_sel=at(9))
    order = list(good)

    def fold(**kw):
        d = dict(good, **kw)
        return lib.woft_flow_chain_fold(*[d[n] for n in order], None)

    plane = 4 * h * w
    bad = [dict(step_flow=None), dict(best_flow=None), dict(best_cost=None), dict(best_vis=None), dict(best_sel=None),
           # a partly-null prev triple: every mix but all / none
           dict(prev_flow=None), dict(prev_cost=None), dict(prev_vis=None), dict(prev_flow=None, prev_cost=None),
           dict(prev_flow=None, prev_vis=None), dict(prev_cost=None, prev_vis=None),
           # aliasing: the running best shares bytes with an input, or with itself
           dict(best_cost=good["prev_cost"]), dict(best_vis=good["prev_vis"]), dict(best_flow=good["prev_flow"]),
           dict(best_flow=good["step_flow"]), dict(best_flow=good["step_flow"] + plane), dict(best_flow=good["step_flow"] - plane),
           dict(best_cost=good["step_flow"] + 2 * plane - 4), dict(best_sel=good["step_mlogit"]), dict(best_vis=good["step_wlogit"]),
           dict(best_sel=good["prev_flow"] + plane), dict(best_vis=good["best_cost"]), dict(best_cost=good["best_flow"] + plane),
           dict(best_sel=good["best_vis"] + 4), dict(prev_flow=None, prev_cost=None, prev_vis=None, best_flow=good["step_flow"]),
           # a bad side
           dict(h=0), dict(w=0), dict(h=-1), dict(w=-5), dict(h=(1 << 24) + 1), dict(w=(1 << 24) + 1),
           # k, unit_cost, vis_thr
           dict(k=-1), dict(k=128), dict(k=1 << 20), dict(unit_cost=NAN), dict(unit_cost=-0.5), dict(unit_cost=-INF),
           dict(vis_thr=-0.01), dict(vis_thr=1.01), dict(vis_thr=NAN), dict(vis_thr=INF)]
    for kw in bad:
        assert fold(**kw) == -1, kw


def test_lazy_exports():
    import woft_amd
    from woft_amd import multiflow
    assert woft_amd.chain_fold is multiflow.chain_fold and woft_amd.MultiFlowTracker is multiflow.MultiFlowTracker
    with pytest.raises(AttributeError):
        woft_amd.no_such_name


def test_python_layers_reject_bad_constants_before_any_device_work():
    import torch
    from woft_amd import chain_fold
    f = torch.zeros(2, 4, 4)
    for kw, match in ((dict(k=-1), "k must"), (dict(k=128), "k must"), (dict(k=0, vis_thr=1.5), "vis_thr"),
                      (dict(k=0, vis_thr=NAN), "vis_thr"), (dict(k=0, unit_cost=-1.0), "unit_cost"),
                      (dict(k=0, unit_cost=NAN), "unit_cost")):
        with pytest.raises(ValueError, match=match):
            chain_fold(None, None, (f,), **kw)
    with pytest.raises(ValueError, match=r"\(2, H, W\)"):
        chain_fold(None, None, (torch.zeros(3, 4, 4),), 0)
    with pytest.raises(ValueError, match="step is"):
        chain_fold(None, None, (f, None, None, None), 0)


# ---- construction ---------------------------------------------------------------------------------------------------------------
class _FakeProvider:
    """Records its calls; a 'flow' is a zero map whose first pixel names the frames it connects (frames are filled with their
    index, so the index is read back from the image)."""

    def __init__(self, **config):
        self.C = SimpleNamespace(**config)
        self.pinned, self.calls = None, []

    def pin_source(self, img):
        self.pinned = img

    def compute_flow(self, src, dst, mode=None, do_sigmoid=None, borrow=None, **kw):
        import torch
        assert mode == "flow" and do_sigmoid is False and borrow is True
        self.calls.append((src, kw))
        h, w = src.shape[:2]
        flow = torch.zeros(2, h, w)
        flow[0, 0, 0], flow[1, 0, 0] = int(src[0, 0, 0]), int(dst[0, 0, 0])
        return flow, None


@pytest.mark.parametrize("deltas", [(), [], (0,), (-1,), (128,), (1, 1), (None, None), (1.0,), ("1",), (True,),
                                    (None, 1, 2, 3, 4, 5, 6, 7, 8), 5, (1, None, 1)])
def test_bad_deltas_raise_at_construction(deltas):
    from woft_amd import MultiFlowTracker
    with pytest.raises(ValueError, match="deltas"):
        MultiFlowTracker(_FakeProvider(), deltas=deltas)


@pytest.mark.parametrize("kw,match", [(dict(vis_thr=-0.1), "vis_thr"), (dict(vis_thr=1.1), "vis_thr"), (dict(vis_thr=NAN), "vis_thr"),
                                      (dict(unit_cost=-1), "unit_cost"), (dict(unit_cost=NAN), "unit_cost"),
                                      (dict(iters=0), "iters"), (dict(iters=2.5), "iters")])
def test_bad_constants_raise_at_construction(kw, match):
    from woft_amd import MultiFlowTracker
    with pytest.raises(ValueError, match=match):
        MultiFlowTracker(_FakeProvider(), **kw)


def test_weights_postprocessing_fn_is_refused():
    from woft_amd import MultiFlowTracker
    with pytest.raises(NotImplementedError, match="weights_postprocessing_fn"):
        MultiFlowTracker(_FakeProvider(weights_postprocessing_fn=lambda x: x))
    trk = MultiFlowTracker(_FakeProvider(weights_postprocessing_fn=None), deltas=[None, 127, 3], iters=4)
    assert trk.deltas == (None, 127, 3) and trk.reach == 127 and trk.iters == 4 and (trk.vis_thr, trk.unit_cost) == (0.5, 1.0)
    with pytest.raises(RuntimeError, match="init"):
        trk.track(np.zeros((8, 8, 3), np.uint8))


# ---- the schedule and the ring --------------------------------------------------------------------------------------------------
def _fake_tracker(monkeypatch, **kw):
    import torch
    from woft_amd import multiflow
    monkeypatch.setattr(multiflow.MultiFlowTracker, "DEVICE", "cpu")
    prov = _FakeProvider()
    trk = multiflow.MultiFlowTracker(prov, **kw)
    log = []

    def fold(best, prev, flow, wl, ml, k, vis_thr, unit_cost, first):
        assert wl is None and ml is None and first == (best is None) and (vis_thr, unit_cost) == (trk.vis_thr, trk.unit_cost)
        log.append((int(flow[0, 0, 0]), int(flow[1, 0, 0]), k, prev is not None))
        h, w = flow.shape[1:]
        return best or (torch.zeros(2, h, w), torch.zeros(h, w), torch.ones(h, w), torch.zeros(h, w, dtype=torch.int32))
    trk._fold = fold
    return trk, prov, log


def _frame(t):
    return np.full((8, 16, 3), t, np.uint8)


def test_default_schedule_and_ring_eviction(monkeypatch):
    """(source frame, target frame, k, chained) of every fold at frames 1, 2, 3, 5 and 33: a delta of exactly t chains through
    frame 0's stored identity result; the ring holds what the largest delta can still reach, nothing older."""
    trk, prov, log = _fake_tracker(monkeypatch)
    trk.init(_frame(0))
    assert prov.pinned is trk._template and sorted(trk._ring) == [0]
    ident = trk._ring[0][1]
    assert not ident[0].any() and not ident[1].any() and (ident[2] == 1).all() and tuple(ident[0].shape) == (2, 8, 16)
    want = {1: [(0, 1, 0, False), (0, 1, 1, True)],
            2: [(0, 2, 0, False), (1, 2, 1, True), (0, 2, 2, True)],
            3: [(0, 3, 0, False), (2, 3, 1, True), (1, 3, 2, True)],
            5: [(0, 5, 0, False), (4, 5, 1, True), (3, 5, 2, True), (1, 5, 3, True)],
            33: [(0, 33, 0, False), (32, 33, 1, True), (31, 33, 2, True), (29, 33, 3, True), (25, 33, 4, True), (17, 33, 5, True),
                 (1, 33, 6, True)]}
    for t in range(1, 36):
        del log[:], prov.calls[:]
        out = trk.track(_frame(t))
        assert out.frame_index == t and tuple(out.flow.shape) == (2, 8, 16) and tuple(out.sel.shape) == (1, 8, 16)
        assert out.occluded.dtype.is_floating_point is False and tuple(out.cost.shape) == tuple(out.vis.shape) == (1, 8, 16)
        if t in want:
            assert log == want[t], t
        assert [(s, k) for s, _, k, _ in log] == [(s, k) for k, s, _ in trk.schedule(t)]
        # template flows come from the pinned object itself, every other source from the ring; no `iters` is passed by default
        for (src, kw), (s, _, _, _) in zip(prov.calls, log):
            assert (src is prov.pinned) == (s == 0) and kw == {}
        assert sorted(trk._ring) == list(range(max(0, t + 1 - 32), t + 1)), t
        assert len(trk._ring) <= 32
    # stored frames and results are the tracker's own: no entry shares memory with another, none is what the caller got
    ptrs = [x.data_ptr() for img, res in trk._ring.values() for x in (img,) + tuple(res)]
    assert len(set(ptrs)) == len(ptrs) and out.flow.data_ptr() not in ptrs and out.cost.data_ptr() not in ptrs
    trk.reset()
    assert trk._ring == {} and trk._template is None and trk.frame_index is None


def test_other_schedules(monkeypatch):
    trk, prov, log = _fake_tracker(monkeypatch, deltas=(None,), iters=3)
    trk.init(_frame(0))
    for t in (1, 2, 3):
        trk.track(_frame(t))
    assert log == [(0, 1, 0, False), (0, 2, 0, False), (0, 3, 0, False)] and trk._ring == {}       # (nothing to reach: nothing kept)
    assert all(kw == dict(iters=3) for _, kw in prov.calls)
    trk, prov, log = _fake_tracker(monkeypatch, deltas=(2, 1))                                       # (fold order = the order given)
    trk.init(_frame(0))
    for t in (1, 2, 3):
        trk.track(_frame(t))
    assert log == [(0, 1, 1, True), (0, 2, 0, True), (1, 2, 1, True), (1, 3, 0, True), (2, 3, 1, True)]
    assert sorted(trk._ring) == [2, 3]
    trk, prov, log = _fake_tracker(monkeypatch, deltas=(3,))        # (frames 1 and 2: no candidate -> the empty result, stored)
    trk.init(_frame(0))
    out = trk.track(_frame(1))
    assert log == [] and (out.sel == -1).all() and out.flow.isnan().all() and out.cost.isinf().all() and out.occluded.all()
    trk.track(_frame(2))
    trk.track(_frame(3))
    assert log == [(0, 3, 0, True)]


# ---- the restatement by hand ----------------------------------------------------------------------------------------------------
def test_restatement_by_hand():
    """2 x 3.  Candidate 0: the template itself, zero flow, both logits 0 -> cost ln 2, vis 0.5 (not below the threshold 0.5).
    Candidate 1: prev flow (1, 0), cost 0.1, vis 1; step flow (2x + 10y, -x) (bilinear reproduces it), unit cost 0.25 -> valid in
    columns 0 and 1 with flow (1 + 2(x+1) + 10y, -(x+1)), cost 0.35: cheaper, wins there.  Candidate 2: prev flow (0.5, 0.5), cost 0,
    vis 0.4, unit cost 0: valid at (0, 0) and (1, 0) only, the cheapest of all but occluded: loses to both."""
    h, w = 2, 3
    ys, xs = np.mgrid[:h, :w].astype(np.float32)
    z, one = np.zeros((h, w), np.float32), np.ones((h, w), np.float32)
    lin = np.stack([2 * xs + 10 * ys, -xs]).astype(np.float32)
    c0 = (None, (np.stack([z, z]), z, z))
    c1 = ((np.stack([one, z]), 0.1 * one, one), (lin, None, None))
    c2 = ((np.stack([0.5 * one, 0.5 * one]), z, 0.4 * one), (lin, None, None))
    for dtype in (np.float64, np.float32):
        b = MH.fold(None, *c0, k=0, dtype=dtype)
        assert (b["sel"] == 0).all() and not b["flow"].any() and np.allclose(b["cost"], math.log(2), rtol=0, atol=1e-6)
        assert (b["vis"] == 0.5).all()
        m = dict(cost=np.inf, vis=np.inf)
        b = MH.fold(b, *c1, k=1, unit_cost=0.25, dtype=dtype, margins=m)
        assert b["sel"].tolist() == [[1, 1, 0], [1, 1, 0]]
        assert b["flow"][0].tolist() == [[3, 5, 0], [13, 15, 0]] and b["flow"][1].tolist() == [[-1, -2, 0], [-1, -2, 0]]
        assert np.allclose(b["cost"][:, :2], 0.35, rtol=0, atol=1e-6) and (b["vis"][:, :2] == 1).all() and (b["vis"][:, 2] == 0.5).all()
        assert abs(m["cost"] - (math.log(2) - 0.35)) < 1e-6 and m["vis"] == 0.5
        keep = {n: v.copy() for n, v in b.items()}
        b2 = MH.fold(b, *c2, k=2, unit_cost=0.0, dtype=dtype)
        assert all(np.array_equal(b2[n], keep[n], equal_nan=True) for n in keep)
        assert all(np.array_equal(b[n], keep[n], equal_nan=True) for n in keep)         # (the input best is left alone)
        # candidate 2 alone: sampled at (x + 0.5, 0.5): flow 0.5 + (2(x+.5) + 5, -(x+.5)); elsewhere the empty pixel
        b = MH.fold(None, *c2, k=2, unit_cost=0.0, dtype=dtype)
        assert b["sel"].tolist() == [[2, 2, -1], [-1, -1, -1]]
        assert b["flow"][:, 0, :2].tolist() == [[6.5, 8.5], [0.0, -1.0]] and np.isnan(b["flow"][:, b["sel"] < 0]).all()
        assert np.isposinf(b["cost"][b["sel"] < 0]).all() and not b["vis"][b["sel"] < 0].any()
        assert (b["cost"][0, :2] == 0).all() and np.allclose(b["vis"][0, :2], 0.4, rtol=0, atol=1e-7)
        # the visible candidate replaces the occluded one although it is dearer
        b = MH.fold(b, *c0, k=0, dtype=dtype)
        assert (b["sel"] == 0).all()


def test_generated_cases_have_the_margins_the_recipe_promises():
    """The figures of DESIGN.md section 18: far from any decision that rounding could turn, every candidate wins its share, some
    pixels have no valid candidate, and fp32 arithmetic selects the same chain everywhere."""
    for h, w, K in MH.CASES:
        cands = MH.make_case(h, w, K)
        b64, m = MH.fold_all(cands)
        b32, _ = MH.fold_all(cands, dtype=np.float32)
        assert m["vis"] >= 0.15 and (K == 1 or m["cost"] >= 0.42), (h, w, K, m)
        assert np.array_equal(b64["sel"], b32["sel"]) and (b64["sel"] < 0).any() and (b64["sel"] >= 0).any()
        share = [(b64["sel"] == k).sum() / max(1, (b64["sel"] >= 0).sum()) for k in range(K)]
        assert min(share) > 0.5 / K, (h, w, K, share)
