"""Training of the weight head on HIP: the kernels of csrc/wh_train.hip against the float64 restatement
(tests/wh_train_host.py), and RAFTWrapper.weight_head_parameters / weights_at / sync_weight_head on the 128x160 golden pair.

Accuracy rule (section 15's): error of a gradient tensor = max |g - g64| / max |g64| against float64 torch autograd of the
restatement on the same float32 inputs; yardstick = the same restatement through float32 torch autograd on the CPU; the
kernels' error must not exceed 4 x the yardstick, floor 1e-6.  Run with -s for the table of (kernel, float32 yardstick) pairs.
Determinism, the sync and the no-regression checks compare bytes.  The NaN some cases place beyond a count are values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wh_train_host as host  # noqa: E402
import pytracking.utils.least_squares_H as L  # noqa: E402  (the shim's import path, as configs use it)
from oracle import hfit_ref  # noqa: E402
from woft_amd import synth  # noqa: E402

FACTOR, FLOOR = 4.0, 1e-6
NAMES = ("w0", "b0", "w2", "b2", "w4", "b4", "w6", "b6")
_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for case, name, err, e32 in _TABLE:
        print(f"\n[wh train] {case} {name}: kernel {err:.3e}, float32 yardstick {e32:.3e}")


def _check(case, got, g64, g32, names=NAMES):
    for name, g, r64, r32 in zip(names, got, g64, g32):
        g = g.detach().cpu()
        assert g.shape == r64.shape and bool(torch.isfinite(g).all()), (case, name)
        err, e32 = host.rel_err(g, r64), host.rel_err(r32, r64)
        _TABLE.append((case, name, err, e32))
        print(f"[wh train] {case} {name}: kernel {err:.3e}, float32 yardstick {e32:.3e}")
    for case_, name, err, e32 in _TABLE[-len(names):]:
        assert err <= max(FACTOR * e32, FLOOR), f"{case_} {name}: kernel {err:.3e}, float32 yardstick {e32:.3e}"


def _check_values(case, v, v64, tol=2e-5):
    """Forward values (not a gradient: the 4 x rule is not theirs): three layers of fp32 fma chains of K <= 1152 products, each
    within sqrt(K) * 2^-24 = 2e-6 of its sum of magnitudes for rounding errors of random sign; 2e-5 of the largest value."""
    err = host.rel_err(v, v64)
    print(f"[wh train] {case} forward values: {err:.3e}")
    assert err <= tol, (case, err)


# ---- kernel level -----------------------------------------------------------------------------------------------------------
def _x8(x5):
    n = x5.shape[0]
    x8 = torch.zeros(n, 81, 8)
    x8[:, :, :5] = x5.permute(0, 2, 3, 1).reshape(n, 81, 5)
    return x8.cuda()


def _head_autograd(x5, params, g_win, dtype):
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    wl = host.head(x5.to(dtype), ps)[3]
    (wl * g_win.to(dtype)).sum().backward()
    return wl.detach(), [p.grad for p in ps]


def _head_device(x5, params, g_win, index, P):
    """head_forward + head_backward on the device for the windows x5, upstream gradient g_win per window, scattered through a
    (P,) map at `index` as the provider does."""
    from woft_amd import ops, wh_train
    n = x5.shape[0]
    z = lambda *s: torch.zeros(*s, device="cuda")
    x8 = _x8(x5)
    dev = [p.cuda() for p in params]
    acts, gbufs, out = [z(n, 81, 128) for _ in range(3)], [z(n, 81, 128) for _ in range(2)], z(n)
    wh_train.head_forward(x8, n, dev[:7], acts, out)
    g_wlow = z(P)
    g_wlow[index.long().cuda()] = g_win.cuda()
    grads = [z(*p.shape) for p in params]
    ws, ws64 = z(ops.wh_wgrad_ws_floats(n, 128)), torch.zeros(-(-n // ops.WH_TRAIN_CHUNK) * 129, dtype=torch.float64, device="cuda")
    wh_train.head_backward(x8, n, (dev[2], dev[4], dev[6]), acts, g_wlow, index.cuda(), gbufs, ws, ws64, grads)
    torch.cuda.synchronize()
    return (out + dev[7]).cpu(), [g.cpu() for g in grads], [a.cpu() for a in acts]


def _head_case(kind):
    from woft_amd import ops
    g = torch.Generator().manual_seed({"1": 11, "5": 12, "chunk+1": 13, "leak": 14, "relu0": 15}[kind])
    n = {"1": 1, "5": 5, "chunk+1": ops.WH_TRAIN_CHUNK + 1, "leak": 2, "relu0": 3}[kind]
    x5 = torch.randn(n, 5, 9, 9, generator=g)
    params = host.random_params(g)
    g_win = torch.randn(n, generator=g)
    if kind == "leak":            # two windows adjacent in memory: the second with a zero gradient and huge inputs
        x5[1] *= 1e4
        g_win[1] = 0.0
    if kind == "relu0":           # activations planted at exactly 0: a zero window under a zero first bias
        x5[0] = 0.0
        params[1].zero_()
    index = torch.randperm(40, generator=g)[:n].sort().values.to(torch.int32)
    return x5, params, g_win, index


@pytest.mark.parametrize("kind", ["1", "5", "chunk+1", "leak", "relu0"])
def test_head_kernels_against_float64_autograd(kind):
    """Forward values and every parameter gradient of the three conv layers + closing conv + mean, full random upstream."""
    x5, params, g_win, index = _head_case(kind)
    wl64, g64 = _head_autograd(x5, params, g_win, torch.float64)
    wl32, g32 = _head_autograd(x5, params, g_win, torch.float32)
    wl, got, acts = _head_device(x5, params, g_win, index, 40)
    _check_values(f"head n_win={kind}", wl, wl64)
    _check(f"head n_win={kind}", got, g64, g32)
    if kind == "relu0":
        assert float(acts[0][0].abs().max()) == 0.0       # the planted zeros are there: pre-activation exactly 0, gate closed


def _upsample_case(crop):
    """hf x wf = 17 x 20 cells (a 132 x 156 image under 'RAFT' padding: top = left = 2; or 136 x 160 uncropped): points on all four
    borders and corners, duplicates, many points in one cell, NaN beyond the count."""
    g = torch.Generator().manual_seed(21 + crop[0])
    hf, wf = 17, 20
    h, w = 8 * hf - 2 * crop[0], 8 * wf - 2 * crop[1]
    n_max, n = 96, 80
    pts = torch.stack([torch.randint(0, w, (n_max,), generator=g), torch.randint(0, h, (n_max,), generator=g)], 1).float()
    edge = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [w // 2, 0], [w // 2, h - 1], [0, h // 2], [w - 1, h // 2]]
    pts[:8] = torch.tensor(edge).float()
    pts[8] = pts[9] = pts[3]                                                            # duplicates (of a corner)
    pts[10:30] = torch.tensor([40.0, 48.0]) + torch.randint(0, 6, (20, 2), generator=g)   # many points in one cell
    pts[n:] = float("nan")
    g_out = torch.randn(n_max, generator=g)
    g_out[n:] = float("nan")
    wlow = torch.randn(hf * wf, generator=g)
    mask = torch.randn(hf * wf, 576, generator=g) * 2
    return hf, wf, n_max, n, pts, g_out, wlow, mask


@pytest.mark.parametrize("crop", [(0, 0), (2, 2)])
@pytest.mark.parametrize("do_sigmoid", [False, True])
@pytest.mark.parametrize("listed", [False, True])
def test_upsampling_adjoint(crop, do_sigmoid, listed):
    """woft_convex_weights_at_bwd against the float64 formula; cells that no point reaches are exact zeros."""
    from woft_amd import ops
    hf, wf, n_max, n, pts, g_out, wlow, mask = _upsample_case(crop)
    d = lambda t: t.double()
    g64 = host.upsample_at_bwd(d(g_out[:n]), d(wlow), d(mask), pts[:n], hf, wf, crop, do_sigmoid)
    g32 = host.upsample_at_bwd(g_out[:n], wlow, mask, pts[:n], hf, wf, crop, do_sigmoid)
    index = None
    if listed:                    # every cell a point reaches, plus a few that none does
        index = torch.unique(torch.cat([torch.nonzero(g64).reshape(-1), torch.tensor([0, 5, hf * wf - 1])])).to(torch.int32).cuda()
    out = torch.full((hf * wf,), 7.0, device="cuda")
    count = torch.tensor([n], dtype=torch.int32, device="cuda")
    ops.convex_weights_at_bwd(pts.cuda(), count, n_max, g_out.cuda(), wlow.cuda(), mask.cuda(), hf, wf, crop, out, index=index,
                              do_sigmoid=do_sigmoid)
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool(torch.isfinite(out).all()) and bool((out[g64 == 0] == 0).all())
    _check(f"upsample adjoint crop={crop} sigmoid={do_sigmoid} listed={listed}", [out], [g64], [g32], names=("g_wlow",))
    # forward consistency: the adjoint belongs to woft_convex_weights_at
    wsel = torch.zeros(n_max, device="cuda")
    ops.convex_weights_at(pts.cuda(), count, n_max, wlow.cuda(), mask.cuda(), hf, wf, crop, wsel, do_sigmoid=do_sigmoid)
    want = host.upsample_at(d(wlow), d(mask), pts[:n], hf, wf, crop, do_sigmoid)
    assert float((wsel[:n].cpu().double() - want).abs().max()) <= 1e-5 and bool((wsel[n:] == 0).all())


# ---- provider level ---------------------------------------------------------------------------------------------------------
def _config(sd, **kw):
    from woft_amd.config import Config
    from woft_amd.flow_provider import RAFTWrapper
    c = Config()
    c.of_class = RAFTWrapper
    c.raft_type = kw.pop("raft_type", "weighted")
    c.class_params = Config()
    c.class_params.small = kw.pop("small", False)
    c.class_params.mixed_precision = False
    c.class_params.alternate_corr = False
    c.class_params.weight_head_structure = kw.pop("structure", [(128, 3)] * 3)
    c.class_params.mask_estimation = kw.pop("mask_estimation", False)
    c.class_params.mask_head_structure = kw.pop("mask_head_structure", None)
    c.model = sd
    c.iters = 4
    c.padding_mode = "nopad"
    c.precision = "fp32"
    c.weights_postprocessing_fn = None
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.fixture(scope="module")
def pair(golden_dir):
    g = np.load(golden_dir / "flow_full_128x160_it4.npz")
    return synth.make_state_dict(seed=int(g["seed"])), np.ascontiguousarray(g["img1"]), np.ascontiguousarray(g["img2"])


@pytest.fixture(scope="module")
def prov(pair):
    from woft_amd.flow_provider import RAFTWrapper
    return RAFTWrapper(_config(pair[0]))


def _sobol_pts(n=64, h=128, w=160):
    """n pixels spread over the frame: x from the tracker's 1-D Sobol sequence, y = its index (a Hammersley set -- the 1-D
    sequence alone, used as a pixel index, puts 64 points of a 160-pixel-wide frame into one column)."""
    from woft_amd import presets
    s = presets.sobol_points(n)
    xy = np.stack([np.floor(w * s), np.floor(h * (np.arange(n) + 0.5) / n)], 1)
    return torch.from_numpy(xy.astype(np.float32)).cuda()


def _frozen_inputs(prov, pts):
    """The device's own frozen inputs of the last weights_at(), read back: (x5, index, mask, hf, wf)."""
    plan = prov._wh_flow[0]
    hf, wf = plan.hf, plan.wf
    need = torch.zeros(hf + 2, wf + 2, dtype=torch.bool)
    for x, y in pts.cpu().long().tolist():
        need[(y >> 3):(y >> 3) + 3, (x >> 3):(x >> 3) + 3] = True
    index = torch.nonzero(need[1:-1, 1:-1].reshape(-1)).reshape(-1).to(torch.int32)
    x5 = host.x5_from_rows(plan.corr.t.cpu(), plan.wmean.cpu(), index)
    return x5, index, plan.mask.t.cpu().clone(), hf, wf


def _params_cpu(prov):
    return [p.detach().cpu().clone() for p in prov.weight_head_parameters().values()]


def _zero_grads(prov):
    for p in prov.weight_head_parameters().values():
        p.grad = None


def test_parameters_are_the_checkpoint(prov, pair):
    d = prov.weight_head_parameters()
    assert list(d) == [f"weight_head.net.{i}.{s}" for i in (0, 2, 4, 6) for s in ("weight", "bias")]
    assert d is prov.weight_head_parameters() and all(p is q for p, q in zip(d.values(), prov.weight_head_parameters().values()))
    for k, p in d.items():
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_cuda and p.dtype == torch.float32
        assert torch.equal(p.detach().cpu(), pair[0][k].float()), k
    torch.optim.SGD(list(d.values()), lr=0.1)


@pytest.mark.parametrize("do_sigmoid", [False, True])
def test_weights_at_values_and_gradients(prov, pair, do_sigmoid):
    """Values against compute_flow's full map at the same pixels (2e-3 on the logits, as tests/test_flow_gpu.py; 1e-6 more through
    the sigmoid); gradients against float64 autograd of the restatement fed the device's own frozen inputs."""
    _, img1, img2 = pair
    full = prov.compute_flow(img1, img2, mode="flow", do_sigmoid=do_sigmoid)[1][0]
    pts = _sobol_pts()
    n_max, n = pts.shape[0], pts.shape[0] - 7
    count = torch.tensor([n], dtype=torch.int32, device="cuda")
    _zero_grads(prov)
    w = prov.weights_at(pts, count, do_sigmoid=do_sigmoid)
    assert w.requires_grad and w.shape == (n_max,) and bool((w[n:] == 0).all())
    at = full[pts[:n, 1].long(), pts[:n, 0].long()]
    err = float((w[:n].detach() - at).abs().max())
    print(f"[wh train] weights_at vs the full map, sigmoid={do_sigmoid}: {err:.3e}")
    assert err <= 2e-3 + (1e-6 if do_sigmoid else 0.0)
    with torch.no_grad():
        w0 = prov.weights_at(pts, count, do_sigmoid=do_sigmoid)
    assert not w0.requires_grad and torch.equal(w0, w.detach())
    # (the forward under no_grad re-ran the same launches: the buffers the backward reads hold the same values, but the
    #  graph's generation is gone -- take a fresh graph for the backward)
    w = prov.weights_at(pts, count, do_sigmoid=do_sigmoid)
    g_out = torch.randn(n_max, generator=torch.Generator().manual_seed(5))
    g_out[n:] = float("nan")
    w.backward(g_out.cuda())
    torch.cuda.synchronize()
    got = [p.grad.clone() for p in prov.weight_head_parameters().values()]
    x5, index, mask, hf, wf = _frozen_inputs(prov, pts[:n])
    a = (x5, _params_cpu(prov), index, mask, pts[:n].cpu(), hf, wf, (0, 0), g_out[:n])
    v64, g64 = host.autograd(*a, do_sigmoid=do_sigmoid, dtype=torch.float64)
    v32, g32 = host.autograd(*a, do_sigmoid=do_sigmoid, dtype=torch.float32)
    _check_values(f"provider sigmoid={do_sigmoid}", w[:n], v64)
    _check(f"provider sigmoid={do_sigmoid}", got, g64, g32)
    # determinism: a second backward on the same inputs gives byte-equal gradients
    _zero_grads(prov)
    prov.weights_at(pts, count, do_sigmoid=do_sigmoid).backward(g_out.cuda())
    for p, q in zip(prov.weight_head_parameters().values(), got):
        assert torch.equal(p.grad, q)
    # after the cheap flow as well
    prov.compute_flow(img1, img2, mode="flow", skip_weights=True)
    assert torch.equal(prov.weights_at(pts, count, do_sigmoid=do_sigmoid).detach(), w.detach())


def test_end_to_end_training_chain(prov, pair):
    """weights_at -> find_homography_nonhomogeneous_QR -> torch_reproj_errors -> backward, through the shim's import paths,
    against the same chain in float64 on the CPU (restatement + oracle fit)."""
    _, img1, img2 = pair
    flow = prov.compute_flow(img1, img2, mode="flow", skip_weights=True)[0]
    pts = _sobol_pts()
    pa = pts
    pb = pts + flow[:, pts[:, 1].long(), pts[:, 0].long()].t()
    GT = torch.tensor([[1.01, 0.002, 1.5], [-0.003, 0.99, -0.8], [1e-5, -2e-5, 1.0]])
    _zero_grads(prov)
    w = prov.weights_at(pts, do_sigmoid=True)
    H = L.find_homography_nonhomogeneous_QR(pa[None], pb[None], w[None])
    loss = L.torch_reproj_errors(GT[None].cuda(), H, pa.t()[None]).mean()
    loss.backward()
    torch.cuda.synchronize()
    got = [p.grad.clone() for p in prov.weight_head_parameters().values()]
    x5, index, mask, hf, wf = _frozen_inputs(prov, pts)

    def chain(dtype):
        ps = [p.to(dtype).requires_grad_(True) for p in _params_cpu(prov)]
        ws = host.weights_at(x5.to(dtype), ps, index, mask.to(dtype), pts.cpu(), hf, wf, (0, 0), True)
        Hh = hfit_ref.find_homography_nonhomogeneous_QR(pa.cpu().to(dtype)[None], pb.cpu().to(dtype)[None], ws[None])
        ls = L.torch_reproj_errors(GT[None].to(dtype), Hh, pa.cpu().to(dtype).t()[None]).mean()
        ls.backward()
        return ls.detach().reshape(1), [p.grad for p in ps]
    l64, g64 = chain(torch.float64)
    l32, g32 = chain(torch.float32)
    # (the loss passes through the fp32 fit: H within ~1e-5 of float64 on a 160-pixel frame moves a re-projected point by
    #  ~1e-3 px, against a loss of the order of a pixel)
    _check_values("end to end (loss)", loss.detach().reshape(1), l64, tol=1e-3)
    _check("end to end", got, g64, g32)


def _weights(p, img1, img2, **kw):
    return p.compute_flow(img1, img2, mode="flow", **kw)[1]


def test_sync_weight_head(pair):
    """Perturbed parameters reach inference only through sync_weight_head(); then compute_flow has the bits of a fresh provider
    built from the exported state dict -- eagerly and with graph = True."""
    from woft_amd.flow_provider import RAFTWrapper
    sd, img1, img2 = pair
    gen = torch.Generator().manual_seed(9)
    for graph in (False, True):
        p = RAFTWrapper(_config(sd, graph=graph))
        before = [_weights(p, img1, img2) for _ in range(3)][-1]                 # (graph: captured at the second call, replayed)
        with torch.no_grad():
            for q in p.weight_head_parameters().values():
                q.add_((0.05 * torch.randn(q.shape, generator=gen)).cuda())
        assert torch.equal(_weights(p, img1, img2), before)                      # no sync: the old bits
        p.sync_weight_head()
        after = [_weights(p, img1, img2) for _ in range(3)]
        merged = dict(sd)
        merged.update({k: v.detach().cpu() for k, v in dict(p.weight_head_parameters()).items()})
        fresh = _weights(RAFTWrapper(_config(merged, graph=graph)), img1, img2)
        assert not torch.equal(after[0], before)
        for a in after:
            assert torch.equal(a, fresh)


def test_refusals(pair, golden_dir):
    from woft_amd.flow_provider import RAFTWrapper
    sd, img1, img2 = pair
    p = RAFTWrapper(_config(sd))
    pts = _sobol_pts()
    with pytest.raises(RuntimeError):
        p.weights_at(pts)                                                        # before any flow
    p.compute_flow(img1, img2, mode="flow", skip_weights=True)
    with pytest.raises(ValueError):
        p.weights_at(torch.zeros(2049, 2, device="cuda"))
    stale = p.weights_at(pts)                                                    # a graph whose flow is replaced before its backward
    p.compute_flow(img1, img2, mode="flow", skip_weights=True)
    with pytest.raises(RuntimeError):
        stale.sum().backward()
    small = RAFTWrapper(_config(synth.make_state_dict(seed=1, small=True), small=True))
    other = RAFTWrapper(_config(synth.make_state_dict(seed=1, weight_head_structure=[(64, 3), (64, 3)]), structure=[(64, 3), (64, 3)]))
    masked = RAFTWrapper(_config(synth.make_state_dict(seed=1, mask_head_structure=[(32, 3)]), raft_type="weighted_masked",
                                 mask_estimation=True, mask_head_structure=[(32, 3)]))
    post = RAFTWrapper(_config(sd, weights_postprocessing_fn=lambda t: t))
    for q in (small, other, masked, post):
        for call in (q.weight_head_parameters, q.sync_weight_head, lambda: q.weights_at(pts)):
            with pytest.raises(NotImplementedError):
                call()


def test_inference_is_untouched_by_training_calls(pair):
    """A compute_flow / finish_weights sequence returns byte-equal outputs before and after a weights_at + backward."""
    from woft_amd.flow_provider import RAFTWrapper
    sd, img1, img2 = pair
    p = RAFTWrapper(_config(sd))
    region = np.zeros((128, 160), bool)
    region[40:90, 50:120] = True
    p.pin_source(img1)
    p.pin_weight_region(region)
    pts = torch.tensor([[60, 50], [61, 50], [100, 80], [70, 45], [55, 88], [118, 41], [90, 60], [75, 75]]).float().cuda()
    count = torch.tensor([8], dtype=torch.int32, device="cuda")

    def sequence():
        out = [t.clone() for t in p.compute_flow(img1, img2, mode="TC", do_sigmoid=True)]
        src, dst, w = p.compute_flow(img1, img2, mode="TC", do_sigmoid=True, borrow=True, weight_region=True, defer_weights=8)
        out.append(dst.clone())
        if p.weights_deferred:
            out.append(p.finish_weights(pts, count, 8, out=torch.zeros(8, device="cuda")).clone())
        out += [t.clone() for t in p.compute_flow(img2, img1, mode="flow")]
        return out
    a = sequence()
    p.compute_flow(img1, img2, mode="flow", skip_weights=True)
    p.weights_at(pts, count, do_sigmoid=True).sum().backward()
    b = sequence()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
