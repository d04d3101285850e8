"""Training of the MaskHead on HIP: the kernels of csrc/mh_train.hip against the float64 restatement
(tests/mh_train_host.py), and RAFTWrapper.mask_head_parameters / visibility_at / sync_mask_head on the 128x160 golden pair.

Accuracy rule (section 15's, as tests/test_wh_train_gpu.py): error of a gradient tensor = max |g - g64| / max |g64| against float64
torch autograd of the restatement on the same float32 inputs; yardstick = the same restatement through float32 torch autograd on
the CPU; the kernels' error must not exceed 4 x the yardstick, floor 1e-6.  Forward values: ten times sqrt(K) * 2^-24 with K =
9 * 512 = 4608 products, the longest fma chain of the head = 4e-5 of the largest value.  Run with -s for the table of (kernel,
float32 yardstick) pairs.  Determinism, the sync and the no-regression checks compare bytes.  The NaN some cases place beyond a
count are values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mh_train_host as host  # noqa: E402
from woft_amd import synth  # noqa: E402

FACTOR, FLOOR, VALUE_TOL = 4.0, 1e-6, 4e-5
_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for case, name, err, e32 in _TABLE:
        print(f"\n[mh train] {case} {name}: kernel {err:.3e}, float32 yardstick {e32:.3e}")


def _names(n):
    return [f"{s}{2 * k}" for k in range(n // 2) for s in ("w", "b")]


def _check(case, got, g64, g32):
    names = _names(len(got))
    for name, g, r64, r32 in zip(names, got, g64, g32):
        g = g.detach().cpu()
        assert g.shape == r64.shape and bool(torch.isfinite(g).all()), (case, name)
        err, e32 = host.rel_err(g, r64), host.rel_err(r32, r64)
        _TABLE.append((case, name, err, e32))
        print(f"[mh train] {case} {name}: kernel {err:.3e}, float32 yardstick {e32:.3e}")
    for case_, name, err, e32 in _TABLE[-len(names):]:
        assert err <= max(FACTOR * e32, FLOOR), f"{case_} {name}: kernel {err:.3e}, float32 yardstick {e32:.3e}"


def _check_values(case, v, v64, tol=VALUE_TOL):
    err = host.rel_err(v, v64)
    print(f"[mh train] {case} forward values: {err:.3e}")
    assert err <= tol, (case, err)


# ---- kernel level -----------------------------------------------------------------------------------------------------------
JUNK = 1e4          # what the 'leak' case plants where nothing may be read: finite, so that 0 * JUNK stays 0 and a read shows


def _map(t_nchw, extra_rows=0, extra_cs=0, fill=0.0):
    """(1, c, h, w) -> a device map (h * w + extra_rows, c + extra_cs), the pad rows and pad channels holding `fill`."""
    _, c, h, w = t_nchw.shape
    m = torch.full((h * w + extra_rows, c + extra_cs), fill)
    m[:h * w, :c] = t_nchw[0].permute(1, 2, 0).reshape(h * w, c)
    return m.cuda()


def _head_device(x, split, params, g_low, pad=False):
    """head_forward + head_backward on the device for the input map x (1, cin, hf, wf) -- as two sources of cin / 2 channels
    with `split` -- and the upstream gradient g_low (hf * wf,).  pad: every buffer gets rows beyond the map and channels beyond
    its width, filled with JUNK (the upstream gradient's extra rows: zeros).
    -> (low, grads, acts, g_maps, buffers): values on the host, the buffers as they are on the device."""
    from woft_amd import mh_train, ops
    _, cin, hf, wf = x.shape
    P, L = hf * wf, len(params) // 2 - 1
    er, ec, fill = (7, 32, JUNK) if pad else (0, 0, 0.0)
    if split:
        x0, x1 = _map(x[:, :cin // 2], er, ec, fill), _map(x[:, cin // 2:], er, ec, fill)
    else:
        x0, x1 = _map(x, er, ec, fill), None
    dev = [p.cuda() for p in params]
    widths = [params[2 * k].shape[0] for k in range(L)]
    full = lambda rows, c: torch.full((rows + er, c + ec), fill, device="cuda")
    acts = [full(P, c) for c in widths]
    gbufs = [full(P, max(widths)) for _ in range(2)]
    out = torch.zeros(P + er, device="cuda")
    mh_train.head_forward(x0, x1, hf, wf, dev[:-1], acts, out)
    g_dev = torch.zeros(P + er, device="cuda")
    g_dev[:P] = g_low.cuda()
    grads = [torch.zeros(*p.shape, device="cuda") for p in params]
    ws = torch.zeros(max(ops.mh_wgrad_ws_floats(hf, wf, params[2 * k].shape[1], widths[k]) for k in range(L)), device="cuda")
    ws64 = torch.zeros(-(-P // ops.MH_REDUCE_CHUNK) * 129, dtype=torch.float64, device="cuda")
    mh_train.head_backward(x0, x1, hf, wf, dev[2::2], acts, g_dev, gbufs, ws, ws64, grads)
    torch.cuda.synchronize()
    low = (out[:P] + dev[-1]).cpu()
    return low, [g.cpu() for g in grads], [a.cpu() for a in acts], [g.cpu() for g in gbufs], (x0, x1, out)


HEADS = {"32|32->32": (64, True, (32,)), "256|256->128->128": (512, True, (128, 128)), "32|32->64->32": (64, True, (64, 32)),
         "128->128": (128, False, (128,)), "64->32": (64, False, (32,))}


def _kernel_case(head, hf, wf, seed):
    cin, split, widths = HEADS[head]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, cin, hf, wf, generator=g)
    params = host.random_params(g, cin, widths)
    g_low = torch.randn(hf * wf, generator=g)
    return x, split, params, g_low


def _run_and_check(case, x, split, params, g_low, pad=False):
    low64, g64, _ = host.head_autograd(x, params, g_low, torch.float64)
    low32, g32, _ = host.head_autograd(x, params, g_low, torch.float32)
    low, got, acts, g_maps, bufs = _head_device(x, split, params, g_low, pad=pad)
    _check_values(case, low, low64)
    _check(case, got, g64, g32)
    return low, got, acts, g_maps, bufs


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (8, 33), (16, 20)])
@pytest.mark.parametrize("head", list(HEADS))
def test_head_kernels_against_float64_autograd(head, size):
    """Forward values and every parameter gradient with a full random upstream: a first layer on two sources at the smallest and
    the shipped widths, inner layers 128 -> 128 and 64 -> 32 (as a second layer behind a data gradient, and on their own as a
    single-source layer); maps of one pixel, smaller than a tile, with a row longer than one 32-position tile, and of more than
    one 256-pixel chunk of the closing conv."""
    hf, wf = size
    _run_and_check(f"{head} {hf}x{wf}", *_kernel_case(head, hf, wf, 100 + hf * wf))


def test_one_more_tile_than_a_chunk():
    """MH_TRAIN_CHUNK + 1 tiles: the weight gradient is the fp64 sum of two partials, the second of a single tile."""
    from woft_amd import ops
    hf, wf = ops.MH_TRAIN_CHUNK + 1, 3
    assert hf * -(-wf // ops.MH_TRAIN_TILE) == ops.MH_TRAIN_CHUNK + 1
    _run_and_check(f"chunk+1 {hf}x{wf}", *_kernel_case("32|32->64->32", hf, wf, 7))
    wf = ops.MH_TRAIN_TILE + 1                      # two tiles per row, chunks that end in the middle of a row
    hf = ops.MH_TRAIN_CHUNK // 2 + 1
    _run_and_check(f"chunk+2 {hf}x{wf}", *_kernel_case("64->32", hf, wf, 8))


@pytest.mark.parametrize("transpose", [False, True])
def test_planted_wrap(transpose):
    """1e4-scaled inputs in the last column, the gradient only in the first column (and the transpose of that: first column,
    last column): a tap at x = -1 (x = wf) that read the pixel before (after) it in memory -- the end of the previous row (the
    start of the next) -- would carry 1e4 into gradients of order one.  wf = 7: with two layers the planted column reaches two
    columns, the gradient's column reads three -- they do not meet."""
    hf, wf = 4, 7
    x, split, params, g_low = _kernel_case("32|32->64->32", hf, wf, 21 + transpose)
    big, hot = (0, wf - 1) if transpose else (wf - 1, 0)
    x[:, :, :, big] *= 1e4
    keep = torch.zeros(hf, wf)
    keep[:, hot] = 1.0
    g_low = g_low * keep.reshape(-1)
    low64, g64, _ = host.head_autograd(x, params, g_low, torch.float64)
    _, g32, _ = host.head_autograd(x, params, g_low, torch.float32)
    low, got, _, _, _ = _head_device(x, split, params, g_low)
    col = lambda v: v.reshape(hf, wf)[:, hot]
    _check_values(f"wrap transpose={transpose} (the gradient's column)", col(low), col(low64))
    _check(f"wrap transpose={transpose}", got, g64, g32)
    assert max(float(g.abs().max()) for g in got) < 1e3          # (nothing of the planted scale arrived)


def test_planted_leak():
    """1e4 in every buffer's rows beyond the map and channels beyond the layer's width, a zero upstream gradient there: the
    results are those of the clean buffers, bit for bit, and the planted values are still where they were."""
    hf, wf = 5, 6
    case = _kernel_case("32|32->64->32", hf, wf, 31)
    low_c, got_c, acts_c, _, _ = _head_device(*case)
    low, got, acts, g_maps, (x0, x1, out) = _run_and_check("leak", *case, pad=True)
    P = hf * wf
    assert torch.equal(low, low_c) and all(torch.equal(a, b) for a, b in zip(got, got_c))
    for a, c in zip(acts, (64, 32)):
        assert bool((a[P:] == JUNK).all()) and bool((a[:, c:] == JUNK).all())
    for gm in g_maps:
        assert bool((gm[P:] == JUNK).all()) and bool((gm[:, 64:] == JUNK).all())
    assert bool((out[P:] == 0).all())


def test_planted_relu0():
    """A zero input region under a zero first bias: the first activation is exactly 0 where the whole 3x3 neighbourhood lies in
    the region, the gate (activation > 0) is closed there, and the gradient that reaches those pixels is exactly 0."""
    hf, wf = 6, 7
    x, split, params, g_low = _kernel_case("32|32->64->32", hf, wf, 41)
    x[:, :, :4, :4] = 0.0
    params[1].zero_()
    low, got, acts, g_maps, _ = _run_and_check("relu0", x, split, params, g_low)
    a1 = acts[0].reshape(hf, wf, -1)
    assert float(a1[:3, :3].abs().max()) == 0.0 and float(a1.abs().max()) > 0.0
    # two layers: the closing conv's adjoint went into g_maps[0], the data gradient through layer 1 into g_maps[1]
    g1 = g_maps[1].reshape(hf, wf, -1)
    assert float(g1[:3, :3].abs().max()) == 0.0 and float(g1.abs().max()) > 0.0
    assert bool(((a1 > 0) | (g1 == 0)).all())                   # closed gates everywhere, not only in the planted region


# ---- provider level ---------------------------------------------------------------------------------------------------------
S1, S2 = [(64, 3)], [(128, 3), (128, 3)]


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


def _pts(h, w, n_max=72, n=64):
    """n pixels spread over the frame (a Hammersley set on the tracker's Sobol sequence), the four corners, the middles of the
    last row and the last column and a duplicate among them; NaN beyond n."""
    from woft_amd import presets
    s = presets.sobol_points(n)
    xy = np.stack([np.floor(w * s), np.floor(h * (np.arange(n) + 0.5) / n)], 1).astype(np.float32)
    xy[:6] = [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [w // 2, h - 1], [w - 1, h // 2]]
    xy[6] = xy[3]
    pts = torch.full((n_max, 2), float("nan"))
    pts[:n] = torch.from_numpy(xy)
    return pts.cuda(), torch.tensor([n], dtype=torch.int32, device="cuda"), n


def _frozen_inputs(p):
    """The device's own frozen inputs of the last flow, read back: (x (1, 2 fdim, hf, wf), mask, hf, wf, crop)."""
    plan, crop = p._last.wh
    hf, wf, P = plan.hf, plan.wf, plan.P
    x = torch.cat([plan.f1rows[:P, :256], plan.mh_warped.t[:P, :256]], 1).cpu()
    return x.reshape(hf, wf, 512).permute(2, 0, 1)[None].contiguous(), plan.mask.t.cpu().clone(), hf, wf, crop


def _params_cpu(p):
    return [q.detach().cpu().clone() for q in p.mask_head_parameters().values()]


def _zero_grads(p):
    for q in p.mask_head_parameters().values():
        q.grad = None


def test_parameters_are_the_checkpoint(prov, pair):
    from woft_amd import mh_train
    sd = _sd(pair[0], S1)
    d = prov.mask_head_parameters()
    assert list(d) == list(mh_train.names(1)) and sorted(d) == sorted(k for k in sd if k.startswith("mask_head.net."))
    assert d is prov.mask_head_parameters() and all(a is b for a, b in zip(d.values(), prov.mask_head_parameters().values()))
    for k, q in d.items():
        assert isinstance(q, torch.nn.Parameter) and q.requires_grad and q.is_cuda and q.dtype == torch.float32
        assert torch.equal(q.detach().cpu(), sd[k].float()), k
    torch.optim.SGD(list(d.values()), lr=0.1)


@pytest.mark.parametrize("structure,precision,padded", [(S1, "fp32", False), (S1, "bf16x3", False), (S2, "fp32", False),
                                                        (S2, "bf16x3", False), (S1, "fp32", True)])
def test_visibility_at_values_and_gradients(pair, structure, precision, padded):
    """Logits and sigmoid against float64 autograd of the restatement fed the plan's own fmap1, warped map and upsampling mask;
    with exact-fp32 inference also against compute_flow's full mask at the same pixels (2e-3, section 17's bound for the same
    comparison).  padded: a 132 x 196 image under 'RAFT' padding -- a 136 x 200 network input, crop offset (2, 2)."""
    _, img1, img2 = pair
    kw = {}
    if padded:
        img1, img2 = (np.ascontiguousarray(np.pad(a, ((2, 2), (18, 18), (0, 0)), mode="reflect")) for a in (img1, img2))
        kw["padding_mode"] = "RAFT"
    p = _provider(pair, structure, precision=precision, **kw)
    h, w = img1.shape[:2]
    pts, count, n = _pts(h, w)
    n_max = pts.shape[0]
    case = f"provider {structure} {precision}" + (" padded" if padded else "")
    for do_sigmoid in (False, True):
        full = p.compute_flow(img1, img2, mode="flow")[2][0]
        if padded:
            assert p._last.wh[1] == (2, 2) and (p._last.wh[0].hp, p._last.wh[0].wp) == (136, 200)
        _zero_grads(p)
        v = p.visibility_at(pts, count, do_sigmoid=do_sigmoid)
        assert v.requires_grad and v.shape == (n_max,) and v.dtype == torch.float32 and bool((v[n:] == 0).all())
        if precision == "fp32":
            at = full[pts[:n, 1].long(), pts[:n, 0].long()]
            at = torch.sigmoid(at) if do_sigmoid else at
            err = float((v[:n].detach() - at).abs().max())
            print(f"[mh train] {case}: visibility_at vs the full mask, sigmoid={do_sigmoid}: {err:.3e}")
            assert err <= 2e-3
        with torch.no_grad():
            v0 = p.visibility_at(pts, count, do_sigmoid=do_sigmoid)
        assert not v0.requires_grad and torch.equal(v0, v.detach())
        v = p.visibility_at(pts, count, do_sigmoid=do_sigmoid)          # (a fresh graph: the no_grad call made the first one stale)
        g_out = torch.randn(n_max, generator=torch.Generator().manual_seed(5))
        g_out[n:] = float("nan")
        v.backward(g_out.cuda())
        torch.cuda.synchronize()
        got = [q.grad.clone() for q in p.mask_head_parameters().values()]
        x, mask, hf, wf, crop = _frozen_inputs(p)
        a = (x, _params_cpu(p), mask, pts[:n].cpu(), hf, wf, crop, g_out[:n])
        v64, g64 = host.autograd(*a, do_sigmoid=do_sigmoid, dtype=torch.float64)
        v32, g32 = host.autograd(*a, do_sigmoid=do_sigmoid, dtype=torch.float32)
        _check_values(f"{case} sigmoid={do_sigmoid}", v[:n], v64)
        _check(f"{case} sigmoid={do_sigmoid}", got, g64, g32)


def test_determinism_and_accumulation(prov, pair):
    """Two backward passes give byte-equal .grad; a third accumulates into the existing .grad and does not overwrite it."""
    _, img1, img2 = pair
    pts, count, _ = _pts(128, 160)
    g_out = torch.randn(pts.shape[0], generator=torch.Generator().manual_seed(6)).cuda()
    prov.compute_flow(img1, img2, mode="flow")
    runs = []
    for _ in range(2):
        _zero_grads(prov)
        prov.visibility_at(pts, count, do_sigmoid=True).backward(g_out)
        runs.append([q.grad.clone() for q in prov.mask_head_parameters().values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and all(float(a.abs().max()) > 0 for a in runs[0])
    for q in prov.mask_head_parameters().values():
        q.grad = torch.full_like(q, 0.25)
    prov.visibility_at(pts, count, do_sigmoid=True).backward(g_out)
    for q, g in zip(prov.mask_head_parameters().values(), runs[0]):
        assert torch.equal(q.grad, torch.full_like(q, 0.25) + g)


def _outputs(p, img1, img2):
    return [t.clone() for t in p.compute_flow(img1, img2, mode="flow")]


def test_sync_mask_head(pair):
    """One SGD step reaches inference only through sync_mask_head(): before it -- after any number of visibility_at calls --
    compute_flow returns the bytes it returned before training began; after it the mask has the bytes of a fresh provider built
    from the merged state dict, eagerly and with graph = True, and flow and weights have not moved."""
    from woft_amd.flow_provider import RAFTWrapper
    seed, img1, img2 = pair
    pts, count, n = _pts(128, 160)
    target = (torch.arange(pts.shape[0]) % 2).float().cuda()
    for graph in (False, True):
        p = _provider(pair, S2, graph=graph)
        before = [_outputs(p, img1, img2) for _ in range(3)][-1]              # (graph: captured at the second call, replayed)
        opt = torch.optim.SGD(list(p.mask_head_parameters().values()), lr=0.5)
        for _ in range(2):
            v = p.visibility_at(pts, count, do_sigmoid=True)
        loss = torch.nn.functional.binary_cross_entropy(v[:n], target[:n])
        loss.backward()
        opt.step()
        assert all(torch.equal(a, b) for a, b in zip(_outputs(p, img1, img2), before))      # no sync: the old bytes
        p.sync_mask_head()
        after = [_outputs(p, img1, img2) for _ in range(3)]
        merged = dict(_sd(seed, S2))
        merged.update({k: q.detach().cpu() for k, q in dict(p.mask_head_parameters()).items()})
        fresh = _outputs(RAFTWrapper(_config(merged, structure=S2, graph=graph)), img1, img2)
        assert not torch.equal(after[0][2], before[2])
        for a in after:
            assert all(torch.equal(x, y) for x, y in zip(a, fresh))
            assert torch.equal(a[0], before[0]) and torch.equal(a[1], before[1])


def test_errors(pair):
    from woft_amd.flow_provider import RAFTWrapper, _LastFlow
    seed, img1, img2 = pair
    p = _provider(pair, S1)
    pts, count, _ = _pts(128, 160)
    with pytest.raises(RuntimeError):
        p.visibility_at(pts, count)                                                # before any flow
    p.compute_flow(img1, img2, mode="flow")
    with pytest.raises(ValueError):
        p.visibility_at(torch.zeros(2049, 2, device="cuda"))
    with pytest.raises(TypeError):
        p.visibility_at(pts.cpu())
    with pytest.raises(TypeError):
        p.visibility_at(pts, torch.tensor([3], device="cuda"))                     # an int64 count
    stale = p.visibility_at(pts, count)                                            # a graph whose flow is replaced before its backward
    p.compute_flow(img1, img2, mode="flow")
    with pytest.raises(RuntimeError):
        stale.sum().backward()
    stale = p.visibility_at(pts, count)                                            # ... or that a later visibility_at replaced
    p.visibility_at(pts, count)
    with pytest.raises(RuntimeError):
        stale.sum().backward()
    # what a flow-cache hit leaves behind (a 'weighted_masked' provider itself never takes a flow from the cache, which holds no
    # mask: the state is the one _cached_flow sets)
    p._last = _LastFlow(p._last.low_plan)
    with pytest.raises(RuntimeError):
        p.visibility_at(pts, count)
    refused = [
        (RAFTWrapper(_config(synth.make_state_dict(seed=1), raft_type="weighted")), "raft_type 'weighted'"),
        (RAFTWrapper(_config(synth.make_state_dict(seed=1, weighted=False), raft_type="orig")), "raft_type 'orig'"),
        (RAFTWrapper(_config(_sd(1, [(32, 3)], small=True), structure=[(32, 3)], small=True)), "small model"),
        (RAFTWrapper(_config(_sd(1, [(128, 5)]), structure=[(128, 5)])), "kernel size 5"),
        (RAFTWrapper(_config(_sd(1, [(48, 3)]), structure=[(48, 3)])), "48 channels"),
    ]
    for q, reason in refused:
        for call in (q.mask_head_parameters, q.sync_mask_head, lambda: q.visibility_at(pts, count)):
            with pytest.raises(NotImplementedError, match=reason):
                call()
