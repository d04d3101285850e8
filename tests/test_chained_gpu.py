"""The planar tracker on chained flow, on the GPU: woft_chain_tc against the float64 restatement
(tests/chain_tc_host.py) on the same fp32 inputs -- dst, ok and hist exact, w within the 4 x float32-yardstick rule with its 1e-6
floor --, its null forms as bits, planted non-finite values; chain_correspondences against the operator;
WOFTChained on a stub provider with known affine motions (geometry and plumbing, independent of network weights) and on the real
provider against the same pieces applied by hand.

Measured on the MI355X (`pytest -s` prints them): max |w - ref64| / its bound; the stub sequence's largest corner re-projection
error against the bound 1e-2 px.

    case                 w
    5 x 7                1.8e-08 / 9.4e-07
    9 x 70               3.8e-08 / 1.0e-06
    37 x 131             4.2e-08 / 1.0e-06
    262145 x 1           4.7e-08 / 1.0e-06
    24 x 40 in 29 x 45   3.7e-08 / 1.0e-06
    stub sequence, frames 2..6: 'weighted' 2.0e-06 px, 'weighted_masked' (left half occluded at frame 3) 2.0e-06 px (1.9e-06 px
    at frame 3)
"""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import chain_tc_host as CH  # noqa: E402
import launch_trace as LT  # noqa: E402
from woft_amd import _lib, ops, synth  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
SENTINEL = 7.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_chain_tc(c, want_w=True, use_mask=True, want_hist=True, vis_thr=None):
    """One woft_chain_tc launch on a case of chain_tc_host.make_case, into outputs filled with a sentinel -> numpy dict."""
    _, h, w = c["flow"].shape
    n = h * w
    full = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device="cuda")
    out = (full(2, n), full(1, n) if want_w else None, full(1, n),
           torch.full((ops.CHAIN_HIST,), -5, dtype=torch.int32, device="cuda") if want_hist else None)
    got = ops.chain_tc(cuda(c["flow"]), cuda(c["cost"]), cuda(c["vis"]), cuda(c["sel"]), cuda(c["mask"]) if use_mask else None,
                       c["vis_thr"] if vis_thr is None else vis_thr, want_w=want_w, mask_hw=c["mask"].shape if use_mask else None,
                       out=out)
    return {k: None if t is None else t.cpu().numpy() for k, t in zip(("dst", "w", "ok", "hist"), got)}


def restate(c, use_mask=True, dtype=np.float64, vis_thr=None):
    return CH.chain_tc(c["flow"], c["cost"], c["vis"], c["sel"], c["mask"] if use_mask else None,
                       c["vis_thr"] if vis_thr is None else vis_thr, dtype=dtype)


def check_against_restatement(got, r64, r32, tag):
    """dst bit for bit (the fp32 sum, NaN where invalid), ok and hist exact, w within the rule and exactly 0 where invalid."""
    valid = r64["valid"].reshape(-1)
    assert np.array_equal(np.isnan(got["dst"]), np.isnan(r64["dst"])) and np.array_equal(np.isnan(got["dst"][0]), ~valid)
    assert np.array_equal(bits(got["dst"][:, valid]), bits(r32["dst"][:, valid]))
    assert np.array_equal(bits(got["dst"][:, valid]), bits(r64["dst"][:, valid].astype(np.float32)))
    assert np.array_equal(bits(got["ok"]), bits(r64["ok"]))
    if got["hist"] is not None:
        assert np.array_equal(got["hist"], r64["hist"]), (tag, got["hist"][[0, 1, 127, 128, 129]], r64["hist"][[0, 1, 127, 128, 129]])
    if got["w"] is not None:
        assert not bits(got["w"][0, ~valid]).any()
        g, a, b = got["w"][0, valid].astype(np.float64), r64["w"][0, valid], r32["w"][0, valid].astype(np.float64)
        bound = max(4 * np.abs(b - a).max(), 1e-6 * np.abs(a).max())
        diff = np.abs(g - a).max()
        print(f"{tag}: w {diff:.1e} / {bound:.1e}")
        assert diff <= bound, f"{tag}: w max |got - ref64| {diff:.3e} > {bound:.3e}"


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generated():
    """Per case: the inputs and the float64 / float32 restatements (computed once, left unchanged)."""
    out = {}
    for h, w, K, mask_hw in CH.CASES:
        c = CH.make_case(h, w, K, mask_hw=mask_hw)
        out[(h, w, K, mask_hw)] = dict(c=c, r64=restate(c), r32=restate(c, dtype=np.float32))
    return out


@pytest.mark.parametrize("case", CH.CASES)
def test_kernel_against_the_restatement(generated, case):
    h, w, K, mask_hw = case
    g = generated[case]
    c, r64 = g["c"], g["r64"]
    got = gpu_chain_tc(c)
    check_against_restatement(got, r64, g["r32"], f"{h} x {w}" + (f" in {mask_hw[0]} x {mask_hw[1]}" if mask_hw else ""))
    assert got["hist"].sum() == (c["mask"][:h, :w] != 0).sum()
    assert got["hist"][127] == 1 and got["hist"][CH.INVALID] >= len(CH.PLANTS) - 2 and got["hist"][CH.OCCLUDED] > 0
    at = {(name, float(v)): i for i, name, v in c["planted"]}
    assert got["ok"][0, at[("vis", 0.5)]] == 1                             # vis == vis_thr is not occluded
    for key in (("sel", -1.0), ("sel", 128.0), ("sel", float(2 ** 31 - 1))):
        i = at[key]
        assert got["ok"][0, i] == 0 and np.isnan(got["dst"][:, i]).all() and got["w"][0, i] == 0


def test_null_forms_leave_the_other_outputs_bits_unchanged(generated):
    """w = NULL, tmask = NULL, hist = NULL, one at a time: the remaining outputs have the bits of the full call (hist without a
    mask counts every pixel: against the restatement)."""
    for case in (CH.CASES[1], CH.CASES[4]):
        c = generated[case]["c"]
        full = gpu_chain_tc(c)
        same = lambda a, names: all(np.array_equal(bits(a[n]), bits(full[n])) for n in names)
        no_w = gpu_chain_tc(c, want_w=False)
        assert no_w["w"] is None and same(no_w, ("dst", "ok")) and np.array_equal(no_w["hist"], full["hist"])
        no_hist = gpu_chain_tc(c, want_hist=False)
        assert no_hist["hist"] is None and same(no_hist, ("dst", "w", "ok"))
        no_mask = gpu_chain_tc(c, use_mask=False)
        assert same(no_mask, ("dst", "w", "ok")) and np.array_equal(no_mask["hist"], restate(c, use_mask=False)["hist"])
        assert no_mask["hist"].sum() == case[0] * case[1]
        bare = gpu_chain_tc(c, want_w=False, use_mask=False, want_hist=False)
        assert bare["w"] is None and bare["hist"] is None and same(bare, ("dst", "ok"))


@pytest.mark.parametrize("thr", [0.0, 0.3, 1.0])
def test_other_thresholds(generated, thr):
    """The closed ends of the range and a threshold that is no fp32 number (the kernel and the restatement compare with its fp32
    rounding; the case plants vis == that value)."""
    h, w, K, mask_hw = CH.CASES[1]
    c = CH.make_case(h, w, K, vis_thr=thr)
    r64 = restate(c)
    check_against_restatement(gpu_chain_tc(c), r64, restate(c, dtype=np.float32), f"thr {thr}")
    if thr == 0.0:
        assert r64["hist"][CH.OCCLUDED] == 0
    if thr == 1.0:
        assert r64["ok"].sum() == 1                                        # (the planted vis == 1 alone)


def test_planted_values_change_only_their_own_pixel(generated):
    for case in CH.CASES[:3]:
        h, w, K, mask_hw = case
        planted = generated[case]["c"]
        clean = CH.make_case(h, w, K, mask_hw=mask_hw, plant=False)
        assert not clean["planted"]
        a, b = gpu_chain_tc(planted), gpu_chain_tc(clean)
        rest = np.ones(h * w, bool)
        rest[[i for i, _, _ in planted["planted"]]] = False
        assert rest.sum() == h * w - len(CH.PLANTS)
        for n in ("dst", "w", "ok"):
            assert np.array_equal(bits(a[n][:, rest]), bits(b[n][:, rest])), n
        assert np.isfinite(b["dst"]).all()


# ---- 2. the public function -----------------------------------------------------------------------------------------------------
def test_public_function_on_host_and_device_tensors(generated):
    """chain_correspondences: the bits of ops.chain_tc for a track() result and for a tuple, device and host tensors; host
    tensors in, host tensors out."""
    from woft_amd import chain_correspondences
    case = CH.CASES[4]
    h, w, K, mask_hw = case
    c = generated[case]["c"]
    want = gpu_chain_tc(c)
    want_nomask = gpu_chain_tc(c, use_mask=False, want_w=False)
    for dev in ("cpu", "cuda"):
        T = lambda a: torch.from_numpy(a).to(dev)
        tup = (T(c["flow"]), T(c["cost"])[None], T(c["vis"])[None], T(c["sel"])[None])
        res = SimpleNamespace(flow=tup[0], cost=tup[1], vis=tup[2], sel=tup[3], occluded=None, frame_index=1)
        for result in (tup, res):
            for mask in (c["mask"], c["mask"] != 0, T(c["mask"])):
                got = chain_correspondences(result, mask, vis_thr=c["vis_thr"])
                assert all(getattr(got, n).device.type == dev for n in ("dst", "w", "ok", "hist"))
                assert [tuple(getattr(got, n).shape) for n in ("dst", "w", "ok", "hist")] == [(2, h * w), (1, h * w), (1, h * w), (130,)]
                assert got.hist.dtype == torch.int32 and np.array_equal(got.hist.cpu().numpy(), want["hist"])
                assert all(np.array_equal(bits(getattr(got, n).cpu().numpy()), bits(want[n])) for n in ("dst", "w", "ok"))
            got = chain_correspondences(result, weights=False)
            assert got.w is None and np.array_equal(got.hist.cpu().numpy(), want_nomask["hist"])
            assert np.array_equal(bits(got.dst.cpu().numpy()), bits(want["dst"]))
    with pytest.raises(ValueError, match="vis_thr"):
        chain_correspondences(tup, vis_thr=1.5)
    with pytest.raises(ValueError, match="smaller"):
        chain_correspondences(tup, np.ones((h - 1, w), np.uint8))
    with pytest.raises(ValueError, match="result is"):
        chain_correspondences(tup[:3])


# ---- 3. the tracker on a stub provider: known affine motions --------------------------------------------------------------------
SH, SW, S_FRAMES, S_DELTAS = 48, 64, 6, (None, 1, 2, 4)
BOUND_PX = 1e-2        # fp32 rounding of coordinates < 64 is ~4e-6 per operation; six chain steps of about ten operations each stay
                       # under 1e-3 px; one order of margin.  A tracker that ignored sel / cost would be off by the planted 5 px.


def _motion(t):
    """A_t: frame 0 -> frame t, 3 x 3 float64 affine: rotation, anisotropic scale about (32, 24), a translation along y.  Along
    the column x = 32 the x-displacement stays under 0.25 px over the first frames (the occlusion test needs that, see there)."""
    c, s = np.cos(0.01 * t), np.sin(0.01 * t)
    L = np.array([[c, -s], [s, c]]) @ np.diag([1 + 0.004 * t, 1 - 0.003 * t])
    centre = np.array([32.0, 24.0])
    A = np.eye(3)
    A[:2, :2], A[:2, 2] = L, centre - L @ centre + np.array([0.0, 0.8 * t])
    return A


class _AffineProvider:
    """A flow provider whose frames carry their index in their pixel value and whose flow s -> t is the analytic A_t A_s^-1 p - p
    (float64, stored as fp32).  The flow of the DIRECT candidate -- the first call of every frame: deltas[0] is None, and frame 0
    is both the template and a stored frame, so only the call order tells the two apart -- carries reliability logit -4 and a
    planted offset of 5 px; every other flow is exact with logit +4.  occlude: None, 'left@3' (visibility logit -6 on the left
    half of every flow into frame 3, +6 elsewhere) or 'all' (-6 everywhere)."""
    precision, precision_source = "stub", "stub"

    def __init__(self, cfg, occlude=None):
        self.C, self.occlude, self.pinned, self.calls, self._last_t = cfg, occlude, None, [], None

    def pin_source(self, img):
        self.pinned = img

    def compute_flow(self, src, dst, mode=None, do_sigmoid=None, borrow=None, **kw):
        assert mode == "flow" and do_sigmoid is False and borrow is True and not kw
        s, t = int(src[0, 0, 0]), int(dst[0, 0, 0])
        direct, self._last_t = t != self._last_t, t
        self.calls.append((s, t, direct))
        ys, xs = np.mgrid[:SH, :SW].astype(np.float64)
        M = _motion(t) @ np.linalg.inv(_motion(s))
        flow = np.stack([M[0, 0] * xs + M[0, 1] * ys + M[0, 2] - xs, M[1, 0] * xs + M[1, 1] * ys + M[1, 2] - ys])
        if direct:
            assert s == 0
            flow += np.array([3.0, 4.0])[:, None, None]
        out = [cuda(flow.astype(np.float32)), None]
        if self.C.raft_type != "orig":
            out[1] = torch.full((1, SH, SW), -4.0 if direct else 4.0, device="cuda")
        if self.C.raft_type == "weighted_masked":
            ml = torch.full((1, SH, SW), -6.0 if self.occlude == "all" else 6.0, device="cuda")
            if self.occlude == "left@3" and t == 3:
                ml[:, :, :SW // 2] = -6.0
            out.append(ml)
        return tuple(out)


def _stub_mask():
    m = np.zeros((SH, SW), np.uint8)
    m[12:36, 16:48] = 255
    return m


def _corner_error(Hm, t):
    """Largest distance between H_cur2init and A_t^-1 applied to the mask's four corners."""
    c = np.array([[16, 12, 1], [47, 12, 1], [47, 35, 1], [16, 35, 1.0]]).T
    a, b = Hm @ c, np.linalg.inv(_motion(t)) @ c
    return float(np.abs(a[:2] / a[2] - b[:2] / b[2]).max())


def _stub_run(monkeypatch, raft_type="weighted", occlude=None, config=None, fused=True):
    from pytracking.utils.config import load_config
    from woft_amd.chained import WOFTChained
    monkeypatch.setenv("WOFT_FUSED", "1" if fused else "0")
    conf = load_config(config or ROOT / "pytracking" / "configs" / "WOFT_chained.py")
    conf.flow_config.raft_type = raft_type
    conf.flow_config.of_class = lambda fc: _AffineProvider(fc, occlude)
    conf.chain_deltas = S_DELTAS
    trk = WOFTChained(conf)
    trk.init(np.zeros((SH, SW, 3), np.uint8), _stub_mask())
    return trk, [trk.track(np.full((SH, SW, 3), t, np.uint8)) for t in range(1, S_FRAMES + 1)]


@pytest.fixture(scope="module")
def stub_preset():
    with pytest.MonkeyPatch.context() as patch:
        return _stub_run(patch)


def test_stub_sequence_follows_the_exact_chains(stub_preset):
    trk, res = stub_preset
    assert trk._fused is not None and "tagged" in trk.solver_decision and str(S_DELTAS) in trk.solver_decision
    n_mask = int((_stub_mask() != 0).sum())
    errs = []
    for t, (Hm, meta) in enumerate(res, 1):
        assert not meta.lost and meta.N_lost == 0 and meta.global_H_success and np.array_equal(Hm, meta.H_global_cur2init)
        assert meta.chain_hist.shape == (len(S_DELTAS),) and meta.chain_hist.dtype == np.int64
        assert meta.chain_hist.sum() + meta.chain_invalid + meta.chain_occluded == n_mask == meta.n_kept
        assert (meta.chain_invalid, meta.chain_occluded) == (0, 0)
        errs.append(_corner_error(Hm, t))
        print(f"frame {t}: chain_hist {meta.chain_hist.tolist()}, corner error {errs[-1]:.2e} px")
        if t >= 2:
            assert meta.chain_hist[0] == 0 and errs[-1] <= BOUND_PX, (t, errs[-1])
    assert hasattr(res[0][1], "solver_decision") and not hasattr(res[1][1], "solver_decision")
    # the provider was asked for the schedule's flows, the direct one first
    assert [c[:2] for c in trk.flower.calls] == [(s, t) for t in range(1, S_FRAMES + 1) for _, s, _ in trk.multi.schedule(t)]
    print(f"stub sequence, frames 2..{S_FRAMES}: largest corner error {max(errs[1:]):.2e} px (bound {BOUND_PX} px)")


def test_stub_sequence_unit_costs(monkeypatch):
    """raft_type 'orig': no logits; every step costs chain_unit_cost, w = exp(-chain length), ties go to the earlier fold -- the
    direct candidate, 5 px off, wins everywhere: the tracker reports that pose, consistently."""
    trk, res = _stub_run(monkeypatch, raft_type="orig")
    for t, (Hm, meta) in enumerate(res, 1):
        assert meta.chain_hist[0] == meta.n_kept and meta.chain_hist[1:].sum() == 0 and np.all(np.isfinite(Hm))
        c = np.array([32.0, 24.0, 1.0])
        a, b = Hm @ (_motion(t) @ c + np.array([3.0, 4.0, 0.0])), c
        assert np.abs(a[:2] / a[2] - b[:2]).max() <= BOUND_PX


def test_stub_sequence_with_the_left_half_occluded_at_frame_3(monkeypatch, stub_preset):
    """'weighted_masked' without a visibility_mode.  Along x = 32 the motions move a pixel by less than 0.25 px in x, so for every
    candidate a template pixel samples the visibility logit on its own side of the boundary (the interpolated logit turns
    positive 0.5 px to the right of column 31): the pixels kept at frame 3 are exactly the mask's right half."""
    trk, res = _stub_run(monkeypatch, raft_type="weighted_masked", occlude="left@3")
    m = _stub_mask() != 0
    right, left = int(m[:, SW // 2:].sum()), int(m[:, :SW // 2].sum())
    assert right == left == 384
    errs = []
    for t, (Hm, meta) in enumerate(res, 1):
        want = (right, left, 0) if t == 3 else (right + left, 0, 0)
        assert not meta.lost and (meta.n_kept, meta.chain_occluded, meta.chain_invalid) == want, t
        errs.append(_corner_error(Hm, t))
        if t >= 2:
            assert meta.chain_hist[0] == 0 and errs[-1] <= BOUND_PX, (t, errs[-1])
    print(f"'weighted_masked', left half occluded at frame 3: largest corner error {max(errs[1:]):.2e} px, at frame 3 {errs[2]:.2e} px")
    # the same provider without the occlusion gives the 'weighted' sequence's poses (vis only gates)
    _, plain = _stub_run(monkeypatch, raft_type="weighted_masked")
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(plain, stub_preset[1]))


def test_stub_sequence_everything_occluded_is_lost_without_an_exception(monkeypatch):
    trk, res = _stub_run(monkeypatch, raft_type="weighted_masked", occlude="all")
    for t, (Hm, meta) in enumerate(res, 1):
        assert meta.lost and meta.N_lost == t and not meta.global_H_success and meta.H_global_cur2init is None
        assert meta.n_kept == 0 and meta.chain_occluded == 768 and meta.chain_hist.sum() == 0
        assert np.array_equal(Hm, np.eye(3))                               # the previous pose: the initial one
    trk2, res2 = _stub_run(monkeypatch, raft_type="weighted_masked", occlude="all", fused=False)
    assert trk2._fused is None and all(m.lost and np.array_equal(Hm, np.eye(3)) and m.n_kept == 0 for Hm, m in res2)


def test_stub_sequence_under_an_inline_callable_config(monkeypatch, stub_preset):
    """The standard of the parent's back-end test (test_tracker_gpu.py): a reference-form config recognised by probing runs the
    device back end with the presets config's H bit for bit; its own callables (device back end off) agree within 1e-2 px at the
    corners."""
    inline = ROOT / "tests" / "configs" / "inline_wlsq.py"
    t_dev, r_dev = _stub_run(monkeypatch, config=inline)
    t_call, r_call = _stub_run(monkeypatch, config=inline, fused=False)
    assert t_dev._fused is not None and "probed" in t_dev.solver_decision and t_call._fused is None
    c = np.array([[16, 12, 1], [47, 12, 1], [47, 35, 1], [16, 35, 1.0]]).T
    for t, ((Ha, ma), (Hb, mb), (Hc, mc)) in enumerate(zip(r_dev, r_call, stub_preset[1]), 1):
        assert np.array_equal(Ha, Hc) and ma.lost == mb.lost == mc.lost and ma.N_lost == mb.N_lost and ma.n_kept == mb.n_kept == mc.n_kept
        assert np.array_equal(ma.chain_hist, mb.chain_hist) and np.array_equal(ma.chain_hist, mc.chain_hist)
        a, b = Ha @ c, Hb @ c
        assert np.abs(a[:2] / a[2] - b[:2] / b[2]).max() < 1e-2
        if t >= 2:
            assert _corner_error(Hb, t) <= BOUND_PX


# ---- 4. the tracker on the real provider: plumbing ------------------------------------------------------------------------------
ITERS, MASK_HEAD = 4, [(64, 3)]


def _real_config(raft_type, padding_mode=None, deltas=(None, 1)):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained.py")
    fc = conf.flow_config
    masked = raft_type == "weighted_masked"
    fc.model = synth.make_state_dict(seed=7, weighted=raft_type != "orig", mask_head_structure=MASK_HEAD if masked else None)
    fc.raft_type, fc.iters, fc.precision = raft_type, ITERS, "bf16x3"
    if masked:
        fc.class_params.mask_estimation, fc.class_params.mask_head_structure = True, MASK_HEAD
    if padding_mode:
        fc.padding_mode = padding_mode
    conf.chain_deltas = deltas
    return conf


@pytest.mark.parametrize("raft_type,padding_mode,hw,deltas", [
    ("orig", None, (128, 160), (None, 1)), ("weighted", None, (128, 160), (None, 1)), ("weighted_masked", None, (128, 160), (None, 1)),
    ("weighted", "crop", (131, 163), (None, 1)), ("weighted", None, (128, 160), (2, 1))])
def test_tracker_equals_the_pieces_applied_by_hand(raft_type, padding_mode, hw, deltas):
    """WOFTChained's H of every frame = a separate MultiFlowTracker on a second provider built from the same state dict,
    chain_correspondences, ops.tc_select_vis and the estimator, bit for bit; and again after init() on the same tracker.
    (None, 1) is the issue's case; on seeded random weights its direct candidate wins everywhere, so (2, 1) -- chains only -- is
    run as well."""
    from woft_amd import MultiFlowTracker, chain_correspondences, presets
    Hh, Ww = hw
    template = synth.make_template(Hh, Ww, seq_id=3)
    frames = [synth.make_frame(template, t) for t in (1, 2, 3)]
    mask = synth.make_init_mask(Hh, Ww)
    conf = _real_config(raft_type, padding_mode, deltas)
    trk = conf.tracker_class(conf)
    assert trk._fused is not None and trk._fused["n_draw"] == 500

    def run():
        trk.init(template, mask)
        return [trk.track(f) for f in frames]
    res = run()

    conf2 = _real_config(raft_type, padding_mode, deltas)
    multi = MultiFlowTracker(conf2.flow_config.of_class(conf2.flow_config), deltas=deltas)
    multi.init(template)
    mask_u8 = cuda((mask > 0).astype(np.uint8) * 255)
    sobol = cuda(presets.sobol_points(500).astype(np.float32))
    pose = np.eye(3)
    for t, (f, (Hm, meta)) in enumerate(zip(frames, res), 1):
        out = multi.track(f)
        gh, gw = out.flow.shape[1:]
        assert (gh, gw) == ((Hh // 8 * 8, Ww // 8 * 8) if padding_mode == "crop" else (Hh, Ww))
        corr = chain_correspondences(out, mask, vis_thr=0.5)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        pa, pb, w, res16 = new(1024, 2), new(1024, 2), new(1024), torch.zeros(16, dtype=torch.float32, device="cuda")
        ires = res16.view(torch.int32)
        ops.tc_select_vis(corr.dst, corr.w, mask_u8, None, Hh, Ww, True, sobol, corr.ok, "gate", 0.5, ops.tc_select_ws(gh * gw), pa, pb,
                          w, ires[12:14], grid=(gh, gw))
        ops.hfit(pa, pb, w, res16[0:9], ires[10:11], count=ires[12:13], reweight=0, huber_k=0.0, n_irls=0)
        ops.inlier_frac(pa, pb, res16[0:9], res16[9:10], thr=5.0, count=ires[12:13])
        host = res16.cpu()
        ih = host.view(torch.int32)
        Hhand = host[0:9].numpy().astype(np.float64).reshape(3, 3)
        usable = int(ih[10]) != 1 and int(ih[13]) >= 4 and bool(np.isfinite(Hhand).all())
        success = usable and bool(np.float32(host[9]) > np.float32(0.2))
        if usable:
            pose = Hhand
        assert meta.n_kept == int(ih[13]) and meta.global_H_success == success and meta.lost == (not success), (raft_type, t)
        assert np.array_equal(Hm, pose), (raft_type, t)
        assert np.array_equal(meta.chain_hist, corr.hist.cpu().numpy()[:2])
        assert meta.chain_hist.sum() + meta.chain_invalid + meta.chain_occluded == int((mask > 0).sum())
        print(f"{raft_type} {padding_mode or ''} {deltas} frame {t}: kept {meta.n_kept}, hist {meta.chain_hist.tolist()}, invalid "
              f"{meta.chain_invalid}, occluded {meta.chain_occluded}, lost {meta.lost}")
    assert any(np.isfinite(Hm).all() and not np.array_equal(Hm, np.eye(3)) for Hm, _ in res)
    again = run()
    assert all(np.array_equal(a[0], b[0]) and a[1].lost == b[1].lost and np.array_equal(a[1].chain_hist, b[1].chain_hist)
               for a, b in zip(again, res))


def test_constructing_the_tracker_leaves_a_plain_compute_flow_as_it_was():
    """The launch trace of a plain compute_flow on the tracker's provider is that of a provider nobody built a tracker around."""
    a, b = LT._pair(128, 160, 2)

    def trace(make_provider):
        real = _lib.load()
        with pytest.MonkeyPatch.context() as patch:
            proxy = LT.LibProxy(real)
            patch.setattr(_lib, "_lib", proxy)
            prov = make_provider(_real_config("weighted"))
            proxy.calls.clear(), proxy._ids.clear()                        # (the trace starts after the construction)
            prov.compute_flow(a, b, mode="flow")
            torch.cuda.synchronize()
        return LT.lines(proxy.calls)
    before = trace(lambda conf: conf.flow_config.of_class(conf.flow_config))
    after = trace(lambda conf: conf.tracker_class(conf).flower)
    assert len(before) > 50 and LT.first_difference(before, after) is None, LT.first_difference(before, after)
