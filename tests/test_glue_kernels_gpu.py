"""Kernel-level tests of the per-frame glue between the flow network and the fit, against float64 / exact references
(tests/fp64_refs.py): the weight head's mean channel (`woft_colsum` + `woft_wh_pack`) and closing 1x1 conv (`woft_wh_reduce`,
also the MaskHead's last layer), the cached-flow epilogue (`woft_flow_to_tc`), the bilinear x8 upsampling with a crop
(`woft_upflow8`), and the correspondence keep rule / selection (`woft_tc_flags`, `woft_tc_select`) on their edge cases.
Tolerances are derived from each kernel's fp32 operations (u = 2^-24); run with -s to see the measured worst error against
each bound."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_refs as R  # noqa: E402

U = R.U32
_STATS = {}


def _note(family, ratio):
    _STATS[family] = max(_STATS.get(family, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam, r in sorted(_STATS.items()):
        print(f"\n[glue fp64] {fam}: worst error / bound {r:.3f}")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from woft_amd import _lib
    _lib.load()
    return _lib


def _within(name, got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = float((err / bound).max()) if err.size else 0.0
    _note(name, ratio)
    assert np.all(err <= bound), f"{name}: worst error {float(err.max()):.3e}, worst error / bound {ratio:.2f}"


# ---- mean channel: colsum + wh_pack ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 425, 1551, 32400])
@pytest.mark.parametrize("C", [256, 128, 96, 300])
def test_colsum_and_mean_against_fp64(lib, P, C):
    """total = sum_q f2[q] in fp64 (any order: |error| <= (P + n_part) u64 sum|f2|), then mean[p] = fp32(alpha) <f1[p], total>
    rounded to fp32: |mean - ref| <= 2u |ref| (alpha's and the result's rounding) + (C + P + n_part) u64 alpha sum_c |f1| |f2|col.
    n_part > P leaves strips empty."""
    g = torch.Generator().manual_seed(P * 1000 + C)
    f1 = (torch.randn(P, C, generator=g) * 3).float()
    f2 = (torch.randn(P, C, generator=g) * 3 + 0.5).float()
    alpha = 1.0 / (math.sqrt(float(C)) * P)
    f1d, f2d = f1.cuda(), f2.cuda()
    ref_total = f2.double().sum(0).numpy()
    abs_total = f2.double().abs().sum(0).numpy()
    if P * P <= 4_000_000:
        ref = R.mean_channel(f1, f2)
    else:                               # (the same mean in its algebraic form: the full P x P volume is 8 GB in fp64)
        ref = (f1.double() @ f2.double().sum(0)).numpy() / (P * math.sqrt(C))
    mag = (f1.double().abs() @ torch.from_numpy(abs_total)).numpy() * alpha
    nwin, ld = 9, 4 * 81 + 12
    lookup = torch.randn(P, ld, generator=g).cuda()
    for n_part in sorted({1, 7, 256, P + 3}):
        ws = torch.full((n_part * C,), float("nan"), dtype=torch.float64, device="cuda")
        total = torch.full((C,), float("nan"), dtype=torch.float64, device="cuda")
        mean = torch.full((P,), float("nan"), device="cuda")
        lib.check(lib.load().woft_colsum(f2d.data_ptr(), P, C, ws.data_ptr(), n_part, total.data_ptr(), lib.stream_ptr()),
                  "woft_colsum")
        lib.check(lib.load().woft_wh_pack(lookup.data_ptr(), ld, f1d.data_ptr(), C, total.data_ptr(), alpha, P, nwin,
                                          mean.data_ptr(), None, lib.stream_ptr()), "woft_wh_pack")
        torch.cuda.synchronize()
        _within("colsum total", total.cpu().numpy(), ref_total, (P + n_part) * R.U64 * abs_total + 1e-300)
        _within("wh mean", mean.cpu().numpy(), ref, 2 * U * np.abs(ref) * (1 + 4 * U) + 2 * (C + P + n_part) * R.U64 * mag)


@pytest.mark.parametrize("nwin,ld", [(9, 4 * 81 + 12), (7, 4 * 49 + 4), (9, 4 * 81)])
def test_wh_pack_layout_bit_exact(lib, nwin, ld):
    """x8[p][t] = (lookup[p][4t .. 4t+3], mean[p], 0, 0, 0), bit for bit, with ld > 4 nwin^2; a mean-only call (x8 = NULL)
    computes the same mean and leaves a poisoned x8 untouched."""
    P, C = 1551, 96
    g = torch.Generator().manual_seed(nwin + ld)
    f1, f2 = torch.randn(P, C, generator=g).cuda(), torch.randn(P, C, generator=g).cuda()
    lookup = torch.randn(P, ld, generator=g).cuda()
    total = f2.double().sum(0).contiguous()
    alpha = 1.0 / (math.sqrt(C) * P)
    t2 = nwin * nwin
    mean = torch.full((P,), float("nan"), device="cuda")
    x8 = torch.full((P, t2, 8), float("nan"), device="cuda")
    lib.check(lib.load().woft_wh_pack(lookup.data_ptr(), ld, f1.data_ptr(), C, total.data_ptr(), alpha, P, nwin,
                                      mean.data_ptr(), x8.data_ptr(), lib.stream_ptr()), "woft_wh_pack")
    mean2 = torch.full((P,), float("nan"), device="cuda")
    x8b = torch.full((P, t2, 8), -7.25, device="cuda")
    lib.check(lib.load().woft_wh_pack(lookup.data_ptr(), ld, f1.data_ptr(), C, total.data_ptr(), alpha, P, nwin,
                                      mean2.data_ptr(), None, lib.stream_ptr()), "woft_wh_pack")
    torch.cuda.synchronize()
    x, lk, m = x8.cpu().numpy(), lookup.cpu().numpy(), mean.cpu().numpy()
    assert np.array_equal(x[:, :, :4], lk[:, :4 * t2].reshape(P, t2, 4))
    assert np.array_equal(x[:, :, 4], np.repeat(m[:, None], t2, 1))
    assert np.all(x[:, :, 5:] == 0)
    assert np.array_equal(mean2.cpu().numpy(), m) and bool((x8b == -7.25).all())


# ---- closing 1x1 conv + patch mean ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [37, 4097])
@pytest.mark.parametrize("nwin2", [1, 49, 81])
@pytest.mark.parametrize("c", [4, 64, 96, 128])
def test_wh_reduce_against_fp64(lib, c, nwin2, P):
    """out[p] = bias + mean_t <w, act[p, t]>.  A lane sums ((w0 a0 + w1 a1) + w2 a2) + w3 a3 for each of its
    I = ceil(nwin2 c / 256) float4 groups into one fp32 accumulator, then 6 shuffle additions, the division by nwin2 and the
    bias: a product passes through at most 1 + 3 + I + 6 + 1 roundings, so with k = I + 12,
    |out - ref| <= k u sum|w act| / nwin2 + 2u |ref|."""
    g = torch.Generator().manual_seed(c * 100 + nwin2 + P)
    act = torch.relu(torch.randn(P, nwin2, c, generator=g)).contiguous()
    w = torch.randn(c, generator=g)
    bias = -0.3125
    out = torch.full((P + 16,), 1234.5, device="cuda")
    act_d, w_d = act.cuda(), w.cuda()
    lib.check(lib.load().woft_wh_reduce(act_d.data_ptr(), c, nwin2, w_d.data_ptr(), bias, P, out.data_ptr(), lib.stream_ptr()),
              "woft_wh_reduce")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[P:] == 1234.5)
    ref, mag = R.wh_reduce(act, w, bias)
    k = math.ceil(nwin2 * c / 256) + 12
    _within("wh_reduce", o[:P], ref, k * U * mag + 2 * U * np.abs(ref))


# ---- cached-flow epilogue -------------------------------------------------------------------------------------------------------
def _ulp32(x):
    """The fp32 spacing at |x| (below 1: the spacing of [0.5, 1), not 1's)."""
    a = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return np.where(a >= 1.0, np.float32(2.0 ** -24), np.spacing(a)).astype(np.float64)


@pytest.mark.parametrize("h,w", [(17, 23), (135, 241), (1, 70000)])
def test_flow_to_tc(lib, h, w):
    """dst = pixel grid + flow and the raw weights are bit-exact against float32 numpy.  The sigmoid 1 / (1 + expf(-x)) is
    within 3 ulp of fp64: expf's 1 ulp, the rounding of the sum and of the quotient each add at most 2^-24 relative, and a
    relative error of 3 * 2^-24 is at most 3 ulp of the result's binade (measured on the MI355X: 2.3 ulp).
    A NULL output leaves the other buffer's neighbours untouched (outputs are poisoned one past the end)."""
    n = h * w
    g = torch.Generator().manual_seed(n)
    flow = (torch.randn(2, n, generator=g) * 40).cuda()
    wt = ((torch.rand(n, generator=g) * 2 - 1) * 30).cuda()
    fl, wn = flow.cpu().numpy(), wt.cpu().numpy()
    i = np.arange(n)
    want_dst = np.stack([(i % w).astype(np.float32) + fl[0], (i // w).astype(np.float32) + fl[1]])

    def run(dst, wout, sig, weights=wt):
        lib.check(lib.load().woft_flow_to_tc(flow.data_ptr(), lib.ptr(weights), h, w, lib.ptr(dst), lib.ptr(wout), sig,
                                             lib.stream_ptr()), "woft_flow_to_tc")
        torch.cuda.synchronize()

    dst = torch.full((2 * n + 8,), -99.0, device="cuda")
    wout = torch.full((n + 8,), -99.0, device="cuda")
    run(dst, wout, 0)
    assert np.array_equal(dst[:2 * n].cpu().numpy(), want_dst.reshape(-1))
    assert np.array_equal(wout[:n].cpu().numpy(), wn)
    assert bool((dst[2 * n:] == -99).all()) and bool((wout[n:] == -99).all())
    wout.fill_(-99.0)
    run(None, wout, 1)
    s = wout[:n].cpu().numpy().astype(np.float64)
    ref = 1.0 / (1.0 + np.exp(-wn.astype(np.float64)))
    _within("flow_to_tc sigmoid (ulp)", np.abs(s - ref) / _ulp32(ref), np.zeros(n), np.full(n, 3.0))
    assert bool((wout[n:] == -99).all())
    dst.fill_(-99.0)
    run(dst, None, 1)
    assert np.array_equal(dst[:2 * n].cpu().numpy(), want_dst.reshape(-1))
    wout.fill_(-99.0)
    run(dst, wout, 1, weights=None)                  # no weights: wout is not written
    assert bool((wout == -99).all())


# ---- bilinear x8 upsampling with a crop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hf,wf,crop,h,w", [(7, 9, (3, 5), 45, 61), (6, 11, (7, 1), 41, 87), (5, 5, (0, 6), 37, 33)])
def test_upflow8_crop_dst_sigmoid(lib, hf, wf, crop, h, w):
    """Flow, dst = window grid + flow and sigmoid(weights) of woft_upflow8 on a cropped window against fp64 bilinear x8
    (align_corners=True) sliced.  Bound, for a source value v interpolated from cells of |v| <= V: the sample position
    carries 2u * max(hf, wf) of rounding (times the neighbour difference <= 2V), the 4-term interpolation and the
    (coords - grid) subtraction ~8u (V + max|coords1| + max(hf, wf)); the flow is that times 8, dst adds u (|dst| + w), and
    the weight logit's error passes through sigmoid' <= 1/4, plus 3 ulp for the sigmoid itself (test_flow_to_tc)."""
    g = torch.Generator().manual_seed(hf * 100 + wf)
    flow = (torch.rand(1, 2, hf, wf, generator=g) * 2 - 1) * 4
    wl = (torch.rand(1, 1, hf, wf, generator=g) * 2 - 1) * 3
    ys, xs = torch.meshgrid(torch.arange(hf, dtype=torch.float32), torch.arange(wf, dtype=torch.float32), indexing="ij")
    coords = (torch.stack([xs, ys])[None] + flow)[0].permute(1, 2, 0).reshape(-1, 2).contiguous()
    flow_eff = coords.T.reshape(1, 2, hf, wf) - torch.stack([xs, ys])[None]       # what the kernel reads back, in fp32
    f_o = torch.full((2 * h * w + 8,), -99.0, device="cuda")
    d_o = torch.full((2 * h * w + 8,), -99.0, device="cuda")
    w_o = torch.full((h * w + 8,), -99.0, device="cuda")
    coords_d, wl_d = coords.cuda(), wl.reshape(-1).contiguous().cuda()
    lib.check(lib.load().woft_upflow8(coords_d.data_ptr(), wl_d.data_ptr(), hf, wf,
                                      crop[0], crop[1], h, w, f_o.data_ptr(), d_o.data_ptr(), w_o.data_ptr(), 1,
                                      lib.stream_ptr()), "woft_upflow8")
    torch.cuda.synchronize()
    for t, m in ((f_o, 2 * h * w), (d_o, 2 * h * w), (w_o, h * w)):
        assert bool((t[m:] == -99).all())
    ref = R.upflow8_crop(flow_eff, crop, h, w)
    m = max(hf, wf)
    fmax, wmax = float(flow_eff.abs().max()), float(wl.abs().max())
    bf = 8 * U * (2 * m * 2 * fmax + 8 * (fmax + float(coords.abs().max()) + m))
    _within("upflow8 flow", f_o[:2 * h * w].cpu().numpy().reshape(2, h, w), ref, np.full(ref.shape, bf))
    gy, gx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dref = np.stack([gx, gy]) + ref
    _within("upflow8 dst", d_o[:2 * h * w].cpu().numpy().reshape(2, h, w), dref, bf + U * (np.abs(dref) + w))
    lw = R.upflow8_crop(wl, crop, h, w)[0] / 8
    sref = 1.0 / (1.0 + np.exp(-lw))
    bw = 0.25 * U * (2 * m * 2 * wmax + 8 * wmax) + 3 * _ulp32(sref)
    _within("upflow8 sigmoid(w)", w_o[:h * w].cpu().numpy().reshape(h, w), sref, bw)


# ---- keep rule and selection ----------------------------------------------------------------------------------------------------
def _select_case(rs, gh, gw, mh, mw, n_keep=None, zero_chunks=()):
    """dst with in / out / NaN / inf / half-way targets, tmask with n_keep kept grid pixels (or random), pwmask."""
    n = gh * gw
    dst = np.stack([rs.uniform(-3, mw + 3, n), rs.uniform(-3, mh + 3, n)]).astype(np.float32)
    sp = rs.choice(n, 60, replace=False)
    dst[0, sp[:6]] = [np.nan, np.inf, -np.inf, mw - 0.5, mw - 1.5, -0.0]
    dst[1, sp[6:12]] = [np.nan, np.inf, -np.inf, mh - 0.5, mh - 1.5, -0.4]
    dst[0, sp[12:20]] = mw - 0.5
    dst[1, sp[20:28]] = mh - 0.5
    tmask = np.zeros((mh, mw), np.uint8)
    if n_keep is None:
        tmask[:] = (rs.uniform(size=(mh, mw)) < 0.97) * 255
        for c in zero_chunks:                      # whole 1024-pixel chunks of the grid with nothing kept
            i = np.arange(c * 1024, min((c + 1) * 1024, n))
            tmask[i // gw, i % gw] = 0
    pw = (rs.uniform(size=(mh, mw)) < 0.9).astype(np.uint8)
    if n_keep is not None:                         # exactly n_keep survivors: in-bounds targets, pwmask 1 there
        dst = np.stack([rs.uniform(0, mw - 1, n), rs.uniform(0, mh - 1, n)]).astype(np.float32)
        pw[:] = 1
        pick = rs.choice(n, n_keep, replace=False)
        tmask[pick // gw, pick % gw] = 255
    return dst, tmask, pw


_CASES = [
    dict(gh=40, gw=56, mh=45, mw=61),                               # crop geometry: grid smaller than the masks
    dict(gh=48, gw=61, mh=51, mw=61),                               # crop in height only (gw == mw)
    dict(gh=64, gw=80, mh=64, mw=80, zero_chunks=(1, 3)),           # empty 1024-pixel chunks
    dict(gh=30, gw=41, mh=33, mw=44, n_keep=0),
    dict(gh=30, gw=41, mh=33, mw=44, n_keep=3),
    dict(gh=30, gw=41, mh=33, mw=44, n_keep=499),
    dict(gh=30, gw=41, mh=33, mw=44, n_keep=500),
    dict(gh=30, gw=41, mh=33, mw=44, n_keep=501),
    dict(gh=96, gw=120, mh=100, mw=128, cap=256),                   # more selected than the output slots
]


@pytest.mark.parametrize("case", range(len(_CASES)))
def test_tc_flags_and_select_edges(lib, case):
    from woft_amd import ops, presets
    kw = dict(_CASES[case])
    cap = kw.pop("cap", 1024)
    rs = np.random.RandomState(100 + case)
    gh, gw, mh, mw = kw["gh"], kw["gw"], kw["mh"], kw["mw"]
    dst, tmask, pw = _select_case(rs, **kw)
    n = gh * gw
    wts = rs.uniform(size=n).astype(np.float32)
    keep = R.keep_rule(dst, tmask, pw, gh, gw)
    if "n_keep" in kw:
        assert int(keep.sum()) == kw["n_keep"]
    dd, tm, pm = torch.from_numpy(dst).cuda(), torch.from_numpy(tmask).cuda(), torch.from_numpy(pw).cuda()
    flags = ops.tc_flags(dd, tm, pm, mh, mw, 1, grid=(gh, gw))
    torch.cuda.synchronize()
    assert np.array_equal(flags.cpu().numpy(), keep)
    u = presets.sobol_points(500).astype(np.float32)
    for use_w in (True, False):
        pa = torch.full((cap + 32, 2), 1e30, device="cuda")
        pb = torch.full((cap + 32, 2), 1e30, device="cuda")
        wo = torch.full((cap + 32,), 1e30, device="cuda")
        cnt = torch.full((2,), -5, dtype=torch.int32, device="cuda")
        ops.tc_select(dd, torch.from_numpy(wts).cuda() if use_w else None, tm, pm, mh, mw, 1, torch.from_numpy(u).cuda(),
                      ops.tc_select_ws(n), pa[:cap], pb[:cap], wo[:cap], cnt, grid=(gh, gw))
        torch.cuda.synchronize()
        rpa, rpb, rwo, m, nk = R.select(dst, wts if use_w else None, tmask, pw, gh, gw, u, cap)
        assert (int(cnt[0]), int(cnt[1])) == (m, nk)
        assert np.array_equal(pa[:m].cpu().numpy(), rpa) and np.array_equal(pb[:m].cpu().numpy(), rpb)
        assert np.array_equal(wo[:m].cpu().numpy(), rwo)
        for t in (pa, pb, wo):
            assert bool((t[m:] == 1e30).all()), "slots past the selected count were written"
