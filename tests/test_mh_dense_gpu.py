"""Training of the MaskHead on dense masks: woft_convex_upsample_bwd against float64 autograd of the dense
restatement (tests/mh_dense_host.py), and RAFTWrapper.visibility_map on the 128x160 golden pair.

Accuracy rule (section 15's, as tests/test_mh_train_gpu.py): error of a gradient tensor = max |g - g64| / max |g64| against float64
torch autograd of the restatement on the same float32 inputs; yardstick = the same restatement through float32 torch autograd on
the CPU; the kernels' error must not exceed 4 x the yardstick, floor 1e-6.  Forward values: section 21's 4e-5 of the largest value.
Run with -s for the table of (kernel, float32 yardstick) pairs.  Equality with visibility_at, determinism, the planted leak and
the no-disturbance check compare bytes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mh_dense_host as host  # noqa: E402
from woft_amd import synth  # noqa: E402

FACTOR, FLOOR, VALUE_TOL = 4.0, 1e-6, 4e-5
JUNK = 1e4          # planted where nothing may be read or kept: finite, so that 0 * JUNK stays 0 and a read shows
_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for case, name, err, e32 in _TABLE:
        print(f"\n[mh dense] {case} {name}: kernel {err:.3e}, float32 yardstick {e32:.3e}")


def _check(case, names, got, g64, g32):
    rows = []
    for name, g, r64, r32 in zip(names, got, g64, g32):
        g = g.detach().cpu()
        assert g.shape == r64.shape and bool(torch.isfinite(g).all()), (case, name)
        rows.append((case, name, host.rel_err(g, r64), host.rel_err(r32, r64)))
        print(f"[mh dense] {case} {name}: kernel {rows[-1][2]:.3e}, float32 yardstick {rows[-1][3]:.3e}")
    _TABLE.extend(rows)
    for case_, name, err, e32 in rows:
        assert err <= max(FACTOR * e32, FLOOR), f"{case_} {name}: kernel {err:.3e}, float32 yardstick {e32:.3e}"


# ---- kernel level -----------------------------------------------------------------------------------------------------------
def _window(hf, wf, cropped):
    """-> (crop, h, w): the whole padded map, or a window that leaves padding on all four sides."""
    return ((2, 3), 8 * hf - 5, 8 * wf - 6) if cropped else ((0, 0), 8 * hf, 8 * wf)


def _inputs(hf, wf, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(hf * wf, 576, generator=g) * 2, torch.randn(hf * wf, generator=g), torch.randn(h * w, generator=g)


def _bwd(mask, wlow, g_up, hf, wf, crop, h, w, do_sigmoid, ld=576, extra_rows=0, prefill=0.0):
    """woft_convex_upsample_bwd on the device: the mask in rows of ld floats with extra_rows after the map, JUNK in every pad
    element; g_wlow and the workspace prefilled.  -> (g_wlow on the host, the mask buffer, the workspace)."""
    from woft_amd import ops
    P = hf * wf
    md = torch.full((P + extra_rows, ld), JUNK)
    md[:P, :576] = mask
    md = md.cuda()
    ws = torch.full((ops.convex_upsample_bwd_ws_floats(hf, wf),), prefill, device="cuda")
    out = torch.full((P,), prefill, device="cuda")
    ops.convex_upsample_bwd(g_up.cuda(), md, wlow.cuda(), hf, wf, crop, h, w, ws, out, do_sigmoid=do_sigmoid)
    torch.cuda.synchronize()
    return out.cpu(), md, ws


@pytest.mark.parametrize("do_sigmoid", [False, True])
@pytest.mark.parametrize("cropped", [False, True])
@pytest.mark.parametrize("size", [(1, 1), (1, 3), (3, 1), (2, 5), (5, 7)])
def test_kernel_against_float64_autograd(size, cropped, do_sigmoid):
    """A map of one cell (every neighbour outside), one row, one column, two rows, and 35 cells (a partial last workgroup of
    four); the whole padded map and a window with padding on all four sides; logits and sigmoid."""
    hf, wf = size
    crop, h, w = _window(hf, wf, cropped)
    mask, wlow, g_up = _inputs(hf, wf, h, w, 300 + 10 * hf + wf)
    a = (wlow, mask, hf, wf, crop, h, w, g_up, do_sigmoid)
    g64, g32 = host.low_grad(*a, dtype=torch.float64), host.low_grad(*a, dtype=torch.float32)
    got, _, _ = _bwd(mask, wlow, g_up, hf, wf, crop, h, w, do_sigmoid)
    _check(f"kernel {hf}x{wf} crop={crop} sigmoid={do_sigmoid}", ["g_wlow"], [got], [g64], [g32])


def test_kernel_is_the_adjoint_of_the_forward_kernel():
    """<g_up, woft_convex_upsample(wlow)> = <woft_convex_upsample_bwd(g_up), wlow> (the logits' map is linear in wlow): the
    adjoint belongs to the kernel the provider's forward runs.  Both sides are float32 sums of h * w and P products of order one:
    1e-5 of the sum of the absolute products."""
    from woft_amd import ops
    hf, wf = 5, 7
    crop, h, w = _window(hf, wf, True)
    mask, wlow, g_up = _inputs(hf, wf, h, w, 77)
    got, md, _ = _bwd(mask, wlow, g_up, hf, wf, crop, h, w, False)
    up = torch.zeros(h * w, device="cuda")
    ops.convex_upsample(torch.zeros(hf * wf, 2, device="cuda"), wlow.cuda(), md, hf, wf, crop, h, w, wout=up)
    lhs, rhs = (g_up.double() * up.cpu().double()), (got.double() * wlow.double())
    assert abs(float(lhs.sum() - rhs.sum())) <= 1e-5 * float(lhs.abs().sum())


@pytest.mark.parametrize("do_sigmoid", [False, True])
def test_planted_leak(do_sigmoid):
    """Mask rows of 640 floats with 1e4 in the 64 pad columns and in 3 rows after the map, 1e4 in g_wlow and in the workspace
    before the call: the bytes of the clean run on rows of 576, and the planted mask values still where they were."""
    hf, wf = 5, 7
    crop, h, w = _window(hf, wf, True)
    mask, wlow, g_up = _inputs(hf, wf, h, w, 78)
    clean, _, _ = _bwd(mask, wlow, g_up, hf, wf, crop, h, w, do_sigmoid)
    got, md, ws = _bwd(mask, wlow, g_up, hf, wf, crop, h, w, do_sigmoid, ld=640, extra_rows=3, prefill=JUNK)
    assert torch.equal(got, clean) and float(clean.abs().max()) > 0
    assert bool((md[hf * wf:] == JUNK).all()) and bool((md[:, 576:] == JUNK).all())
    assert bool((ws != JUNK).all())                            # (every partial was written: none of the prefill is left to be read)


def test_one_hot():
    """g_up = 1 at one pixel, logits: g_wlow is that pixel's nine convex coefficients, in its 3x3 cell neighbourhood and nowhere
    else; they sum to 1 inside the map, and at the corner pixel to the softmax mass of the four neighbours the map holds."""
    hf, wf = 5, 7
    h, w = 8 * hf, 8 * wf
    mask, wlow, _ = _inputs(hf, wf, h, w, 79)

    def run(y, x):
        g_up = torch.zeros(h, w)
        g_up[y, x] = 1.0
        got, _, _ = _bwd(mask, wlow, g_up.reshape(-1), hf, wf, (0, 0), h, w, False)
        return got.reshape(hf, wf)

    got = run(19, 29)                                           # cell (2, 3), fine position (3, 5)
    outside = got.clone()
    outside[1:4, 2:5] = 0
    assert float(outside.abs().max()) == 0.0 and bool((got[1:4, 2:5] > 0).all())
    assert abs(float(got.double().sum()) - 1.0) <= 1e-6
    s = torch.softmax(mask[2 * wf + 3].double().reshape(9, 64)[:, 3 * 8 + 5], 0).reshape(3, 3)
    assert float((got[1:4, 2:5].double() - s).abs().max()) <= 1e-6
    got = run(0, 0)                                             # taps (1, 1), (1, 2), (2, 1), (2, 2) = k 4, 5, 7, 8 lie in the map
    outside = got.clone()
    outside[:2, :2] = 0
    assert float(outside.abs().max()) == 0.0
    s = torch.softmax(mask[0].double().reshape(9, 64)[:, 0], 0)
    assert abs(float(got.double().sum()) - float(s[[4, 5, 7, 8]].sum())) <= 1e-6 and float(s[[4, 5, 7, 8]].sum()) < 1.0


def test_kernel_determinism():
    hf, wf = 5, 7
    crop, h, w = _window(hf, wf, True)
    mask, wlow, g_up = _inputs(hf, wf, h, w, 80)
    a, _, _ = _bwd(mask, wlow, g_up, hf, wf, crop, h, w, True)
    b, _, _ = _bwd(mask, wlow, g_up, hf, wf, crop, h, w, True, prefill=-3.0)
    assert torch.equal(a, b)


# ---- provider level ---------------------------------------------------------------------------------------------------------
S1, S2 = [(32, 3)], [(128, 3), (128, 3)]


def _config(sd, **kw):
    from woft_amd.config import Config
    from woft_amd.flow_provider import RAFTWrapper
    c = Config()
    c.of_class = RAFTWrapper
    c.raft_type = kw.pop("raft_type", "weighted_masked")
    c.class_params = Config()
    c.class_params.small = kw.pop("small", False)
    c.class_params.mixed_precision = False
    c.class_params.alternate_corr = False
    c.class_params.weight_head_structure = [(128, 3)] * 3
    c.class_params.mask_estimation = c.raft_type == "weighted_masked"
    c.class_params.mask_head_structure = kw.pop("structure", None)
    c.model = sd
    c.iters = 4
    c.padding_mode = kw.pop("padding_mode", "nopad")
    c.precision = kw.pop("precision", "fp32")
    c.weights_postprocessing_fn = None
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.fixture(scope="module")
def pair(golden_dir):
    g = np.load(golden_dir / "flow_full_128x160_it4.npz")
    return int(g["seed"]), np.ascontiguousarray(g["img1"]), np.ascontiguousarray(g["img2"])


def _sd(seed, structure, **kw):
    return synth.make_state_dict(seed=seed, mask_head_structure=structure, **kw)


def _provider(pair, structure, **kw):
    from woft_amd.flow_provider import RAFTWrapper
    return RAFTWrapper(_config(_sd(pair[0], structure), structure=structure, **kw))


@pytest.fixture(scope="module")
def prov(pair):
    return _provider(pair, S1)


def _pts(h, w, n=64):
    """n pixels spread over the frame (a Hammersley set on the tracker's Sobol sequence), the four corners, the middles of the
    last row and the last column and a duplicate among them."""
    from woft_amd import presets
    s = presets.sobol_points(n)
    xy = np.stack([np.floor(w * s), np.floor(h * (np.arange(n) + 0.5) / n)], 1).astype(np.float32)
    xy[:6] = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [w // 2, h - 1], [w - 1, h // 2]]
    xy[6] = xy[3]
    return torch.from_numpy(xy).cuda()


def _frozen_inputs(p):
    """The device's own frozen inputs of the last flow, read back: (x (1, 2 fdim, hf, wf), mask, hf, wf, crop)."""
    plan, crop = p._last.wh
    hf, wf, P = plan.hf, plan.wf, plan.P
    x = torch.cat([plan.f1rows[:P, :256], plan.mh_warped.t[:P, :256]], 1).cpu()
    return x.reshape(hf, wf, 512).permute(2, 0, 1)[None].contiguous(), plan.mask.t.cpu().clone(), hf, wf, crop


def _params(p):
    return list(p.mask_head_parameters().values())


def _zero_grads(p):
    for q in _params(p):
        q.grad = None


def _grads(p):
    return [q.grad.clone() for q in _params(p)]


def _names(n):
    return [f"{s}{2 * k}" for k in range(n // 2) for s in ("w", "b")]


@pytest.mark.parametrize("structure,precision,padded", [(S1, "fp32", False), (S1, "bf16x3", False), (S2, "fp32", False),
                                                        (S2, "bf16x3", False), (S1, "fp32", True)])
def test_visibility_map_values_and_gradients(pair, structure, precision, padded):
    """The map has the bytes of visibility_at at 64 pixels (corners, last row, last column), the values and -- for a dense random
    cotangent -- every parameter gradient of float64 autograd of the restatement fed the plan's own fmap1, warped map and
    upsampling mask.  padded: a 132 x 196 image under 'RAFT' padding -- a 136 x 200 network input, crop offset (2, 2)."""
    _, img1, img2 = pair
    kw = {}
    if padded:
        img1, img2 = (np.ascontiguousarray(np.pad(a, ((2, 2), (18, 18), (0, 0)), mode="reflect")) for a in (img1, img2))
        kw["padding_mode"] = "RAFT"
    p = _provider(pair, structure, precision=precision, **kw)
    h, w = img1.shape[:2]
    pts = _pts(h, w)
    case = f"provider {structure} {precision}" + (" padded" if padded else "")
    p.compute_flow(img1, img2, mode="flow")
    if padded:
        assert p._last.wh[1] == (2, 2) and (p._last.wh[0].hp, p._last.wh[0].wp) == (136, 200)
    g_out = torch.randn(h, w, generator=torch.Generator().manual_seed(5))
    for do_sigmoid in (False, True):
        with torch.no_grad():
            at = p.visibility_at(pts, do_sigmoid=do_sigmoid)
        m = p.visibility_map(do_sigmoid=do_sigmoid)
        assert m.shape == (h, w) and m.dtype == torch.float32 and m.is_cuda and m.requires_grad
        assert torch.equal(m.detach()[pts[:, 1].long(), pts[:, 0].long()], at)
        with torch.no_grad():
            m0 = p.visibility_map(do_sigmoid=do_sigmoid)
        assert not m0.requires_grad and m0.grad_fn is None and torch.equal(m0, m.detach())
        m = p.visibility_map(do_sigmoid=do_sigmoid)                # (a fresh graph: the no_grad call made the first one stale)
        _zero_grads(p)
        m.backward(g_out.cuda())
        torch.cuda.synchronize()
        got = _grads(p)
        x, mask, hf, wf, crop = _frozen_inputs(p)
        a = (x, [q.detach().cpu() for q in _params(p)], mask, hf, wf, crop, h, w, g_out)
        v64, g64 = host.autograd_dense(*a, do_sigmoid=do_sigmoid, dtype=torch.float64)
        v32, g32 = host.autograd_dense(*a, do_sigmoid=do_sigmoid, dtype=torch.float32)
        err = host.rel_err(m, v64)
        print(f"[mh dense] {case} sigmoid={do_sigmoid} forward values: {err:.3e}")
        assert err <= VALUE_TOL
        _check(f"{case} sigmoid={do_sigmoid}", _names(len(got)), got, g64, g32)


def test_determinism_and_accumulation(prov, pair):
    """Two backward passes give byte-equal .grad; a third accumulates into the existing .grad and does not overwrite it.  Only
    the head's parameters receive a gradient."""
    _, img1, img2 = pair
    g_out = torch.randn(128, 160, generator=torch.Generator().manual_seed(6)).cuda()
    prov.compute_flow(img1, img2, mode="flow")
    runs = []
    for _ in range(2):
        _zero_grads(prov)
        prov.visibility_map(do_sigmoid=True).backward(g_out)
        runs.append(_grads(prov))
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and all(float(a.abs().max()) > 0 for a in runs[0])
    for q in _params(prov):
        q.grad = torch.full_like(q, 0.25)
    prov.visibility_map(do_sigmoid=True).backward(g_out)
    for q, g in zip(_params(prov), runs[0]):
        assert torch.equal(q.grad, torch.full_like(q, 0.25) + g)


def test_dense_loss_trains_only_required_parameters(prov, pair):
    """The issue's snippet: a BCE-with-logits loss on a valid-pixel selection of the map; a parameter with requires_grad = False
    keeps .grad None, and with none requiring grad the map is a plain tensor."""
    _, img1, img2 = pair
    prov.compute_flow(img1, img2, mode="flow")
    gen = torch.Generator().manual_seed(9)
    target = (torch.rand(128, 160, generator=gen) > 0.5).float().cuda()
    valid = (torch.rand(128, 160, generator=gen) > 0.25).cuda()
    params = _params(prov)
    _zero_grads(prov)
    params[0].requires_grad_(False)
    try:
        logits = prov.visibility_map()
        torch.nn.functional.binary_cross_entropy_with_logits(logits[valid], target[valid]).backward()
        assert params[0].grad is None and all(q.grad is not None and float(q.grad.abs().max()) > 0 for q in params[1:])
        for q in params:
            q.requires_grad_(False)
        assert not prov.visibility_map().requires_grad
    finally:
        for q in params:
            q.requires_grad_(True)
        _zero_grads(prov)


def test_visibility_at_is_not_disturbed(prov, pair):
    """After a visibility_map forward and backward, visibility_at returns the bytes it returned before, values and gradients: the
    two paths share the plan's training buffers."""
    _, img1, img2 = pair
    pts = _pts(128, 160)
    g_pts = torch.randn(pts.shape[0], generator=torch.Generator().manual_seed(7)).cuda()
    prov.compute_flow(img1, img2, mode="flow")
    _zero_grads(prov)
    before = prov.visibility_at(pts, do_sigmoid=True)
    before.backward(g_pts)
    g_before = _grads(prov)
    _zero_grads(prov)
    prov.visibility_map(do_sigmoid=True).backward(torch.ones(128, 160, device="cuda"))
    _zero_grads(prov)
    after = prov.visibility_at(pts, do_sigmoid=True)
    after.backward(g_pts)
    assert torch.equal(after.detach(), before.detach()) and all(torch.equal(a, b) for a, b in zip(_grads(prov), g_before))
    _zero_grads(prov)


def test_errors(pair):
    from woft_amd.flow_provider import RAFTWrapper, _LastFlow
    seed, img1, img2 = pair
    p = _provider(pair, S1)
    pts = _pts(128, 160)
    with pytest.raises(RuntimeError):
        p.visibility_map()                                                         # before any flow
    p.compute_flow(img1, img2, mode="flow")
    stale = p.visibility_map()                                                     # a graph whose flow is replaced before its backward
    p.compute_flow(img1, img2, mode="flow")
    with pytest.raises(RuntimeError):
        stale.sum().backward()
    stale = p.visibility_map()                                                     # ... or that a later visibility_at replaced
    p.visibility_at(pts)
    with pytest.raises(RuntimeError):
        stale.sum().backward()
    stale = p.visibility_map()                                                     # ... or a later visibility_map
    p.visibility_map()
    with pytest.raises(RuntimeError):
        stale.sum().backward()
    stale = p.visibility_at(pts)                                                   # and a visibility_at graph by a visibility_map
    p.visibility_map()
    with pytest.raises(RuntimeError):
        stale.sum().backward()
    p._last = _LastFlow(p._last.low_plan)                                          # what a flow-cache hit leaves behind
    with pytest.raises(RuntimeError):
        p.visibility_map()
    refused = [
        (RAFTWrapper(_config(synth.make_state_dict(seed=1), raft_type="weighted")), "raft_type 'weighted'"),
        (RAFTWrapper(_config(_sd(1, [(32, 3)], small=True), structure=[(32, 3)], small=True)), "small model"),
        (RAFTWrapper(_config(_sd(1, [(128, 5)]), structure=[(128, 5)])), "kernel size 5"),
    ]
    for q, reason in refused:
        with pytest.raises(NotImplementedError, match=reason):
            q.visibility_map()
