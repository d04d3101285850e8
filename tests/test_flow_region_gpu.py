"""Region-restricted launches (woft_conv_params.roi_*, woft_lookup_otf_params.roi_* / smp_*), kernel by kernel: a restricted
launch writes, inside its rectangle, exactly the bits of the whole-map launch and nothing outside it.  A 37 x 53 map (no multiple
of any tile), rectangles: interior and unaligned, one pixel, touching each border, a corner, the whole map."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 37, 53
RECTS = [(5, 7, 9, 18), (20, 30, 1, 1), (0, 10, 6, 20), (30, 10, 7, 20), (10, 0, 9, 11), (10, 40, 9, 13), (29, 36, 8, 17),
         (0, 0, H, W)]
SENTINEL = -77.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from woft_amd import _lib, ops as o
    _lib.load()
    return o


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _inside(rect):
    m = torch.zeros(H, W, dtype=torch.bool)
    m[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]] = True
    return m.reshape(-1).cuda()


def _set_roi(p, rect):
    p.roi_y0, p.roi_x0, p.roi_h, p.roi_w = rect


def _pc(ops, cout, cin, kh, kw, seed, **kw_):
    return ops.pack_conv(_rand(cout, cin, kh, kw, seed=seed, scale=1 / math.sqrt(cin * kh * kw)), _rand(cout, seed=seed + 1, scale=0.1),
                         padding=(kh // 2, kw // 2), **kw_)


def _check(bufs_ref, bufs, masks, what):
    """bufs_ref / bufs: [(tensor (P, C), column slice)], masks: per buffer the pixels its launch had to write."""
    for (ref, cols), (got, _), m in zip(bufs_ref, bufs, masks):
        assert torch.equal(got[m][:, cols], ref[m][:, cols]), f"{what}: inside the rectangle differs from the whole-map launch"
        assert bool((got[~m][:, cols] == SENTINEL).all()), f"{what}: written outside the rectangle"
        rest = torch.ones(got.shape[1], dtype=torch.bool)
        rest[cols] = False
        assert bool((got[:, rest.cuda()] == SENTINEL).all()), f"{what}: written outside its channels"


# (halo, tiles): the register-streamed kernel's instances of the hot path -- 8x16 pixels x 64 / x 128 columns, 4x16 x 128
INSTANCES = [(8, (128, 64)), (8, (128, 128)), (12, None)]


@pytest.mark.parametrize("kh,kw", [(3, 3), (1, 5), (5, 1)])
@pytest.mark.parametrize("halo,tiles", INSTANCES)
@pytest.mark.parametrize("cin", [64, 256])
def test_conv_regb_relu(ops, kh, kw, halo, tiles, cin):
    x = ops.act_from_nchw(_rand(1, cin, H, W, seed=1), cs=cin)
    pc = _pc(ops, 128, cin, kh, kw, 2)
    mk = lambda: torch.full((H * W, 160), SENTINEL, device="cuda")
    ref = mk()
    act = lambda t: ops.Act(t, 1, H, W, 128)
    p0 = ops.conv_params(x, pc, act(ref), co_off=16, epi=1, precision="bf16x3", halo=halo, tiles=tiles)
    assert p0.halo == halo
    ops.run_conv(p0)
    for rect in RECTS:
        out = mk()
        p = ops.conv_params(x, pc, act(out), co_off=16, epi=1, precision="bf16x3", halo=halo, tiles=tiles)
        _set_roi(p, rect)
        ops.run_conv(p)
        torch.cuda.synchronize()
        _check([(ref, slice(16, 144))], [(out, None)], [_inside(rect)], f"relu {kh}x{kw} halo {halo} {tiles} {rect}")


@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)])
@pytest.mark.parametrize("halo,tiles", INSTANCES)
def test_conv_regb_gru_half_step(ops, kh, kw, halo, tiles):
    """GRU_ZR (two outputs, e0) and GRU_Q (e0, e1) with two input sources and per-pixel bias maps, as the update block runs them."""
    E = ops._lib
    h = ops.act_from_nchw(torch.tanh(_rand(1, 128, H, W, seed=3)))
    x = ops.act_from_nchw(_rand(1, 128, H, W, seed=4))
    gz, gq = ops.act_from_nchw(_rand(1, 256, H, W, seed=5, scale=0.2)), ops.act_from_nchw(_rand(1, 128, H, W, seed=6, scale=0.2))
    pzr = ops.pack_conv(_rand(256, 256, kh, kw, seed=7, scale=0.03), None, padding=(kh // 2, kw // 2))
    pq = ops.pack_conv(_rand(128, 256, kh, kw, seed=8, scale=0.03), None, padding=(kh // 2, kw // 2))
    mk = lambda: ops.Act(torch.full((H * W, 128), SENTINEL, device="cuda"), 1, H, W, 128)

    def step(rect):
        z, rh, hn = mk(), mk(), mk()
        a = ops.conv_params(h, pzr, z, x2=x, c_split=128, epi=E.EPI_GRU_ZR, split=128, e0=h, out1=rh, bias_map=gz,
                            precision="bf16x3", halo=halo, tiles=tiles)
        if rect:
            _set_roi(a, rect)
        ops.run_conv(a)
        rin = rh
        if rect:        # (the q conv's halo reads r*h beyond the rectangle: give it the whole-map tensor)
            rin = full[1]
        b = ops.conv_params(rin, pq, hn, x2=x, c_split=128, epi=E.EPI_GRU_Q, e0=h, e1=full[0] if rect else z, bias_map=gq,
                            precision="bf16x3", halo=halo, tiles=tiles)
        if rect:
            _set_roi(b, rect)
        ops.run_conv(b)
        torch.cuda.synchronize()
        return z, rh, hn

    full = None
    full = step(None)
    for rect in RECTS:
        got = step(rect)
        m = _inside(rect)
        _check([(t.t, slice(0, 128)) for t in full], [(t.t, None) for t in got], [m, m, m], f"gru {kh}x{kw} halo {halo} {tiles} {rect}")


@pytest.mark.parametrize("cin", [64, 128])
def test_conv_regb_flowhead(ops, cin):
    """WOFT_EPI_FLOWHEAD: the per-tap partial products of every column-tile plane, inside the rectangle only."""
    x = ops.act_from_nchw(torch.tanh(_rand(1, cin, H, W, seed=9)), cs=(cin + 31) // 32 * 32)
    pc1 = _pc(ops, 256, cin, 3, 3, 10)
    w2 = _rand(2, 256, 3, 3, seed=12, scale=0.02)
    frags = ops.pack_flowhead_frags(w2, 2)
    mk = lambda: torch.full((4 * H * W, 20), SENTINEL, device="cuda")
    ref = mk()
    p0 = ops.flowhead_params(x, pc1, ref, frags, precision="bf16x3")
    assert p0 is not None and p0.halo == 8
    ops.run_conv(p0)
    n = p0._n_planes
    for rect in RECTS:
        out = mk()
        p = ops.flowhead_params(x, pc1, out, frags, precision="bf16x3")
        _set_roi(p, rect)
        ops.run_conv(p)
        torch.cuda.synchronize()
        m = _inside(rect).repeat(n)
        used = slice(0, n * H * W)
        assert torch.equal(out[used][m], ref[used][m]), rect
        assert bool((out[used][~m] == SENTINEL).all()) and bool((out[n * H * W:] == SENTINEL).all()), rect


def test_conv_regb_pair_two_rectangles(ops):
    """woft_conv2d_pair on the register-streamed kernel: each layer its own rectangle (convc2 | convf2 into one buffer)."""
    a1 = ops.act_from_nchw(_rand(1, 256, H, W, seed=13))
    b1 = ops.act_from_nchw(_rand(1, 128, H, W, seed=14))
    c2, f2 = _pc(ops, 192, 256, 3, 3, 15), _pc(ops, 64, 128, 3, 3, 17)
    mk = lambda: torch.full((H * W, 256), SENTINEL, device="cuda")

    def run(ra, rb):
        cf = mk()
        act = ops.Act(cf, 1, H, W, 256)
        qa = ops.conv_params(a1, c2, act, co_off=0, epi=1, precision="bf16x3")
        qb = ops.conv_params(b1, f2, act, co_off=192, epi=1, precision="bf16x3")
        assert ops.pair_ok(qa, qb) and qa.halo == 8
        if ra:
            _set_roi(qa, ra)
        if rb:
            _set_roi(qb, rb)
        ops.run_conv_pair(qa, qb)
        torch.cuda.synchronize()
        return cf

    ref = run(None, None)
    for ra, rb in zip(RECTS, RECTS[1:] + RECTS[:1]):
        got = run(ra, rb)
        ma, mb = _inside(ra), _inside(rb)
        assert torch.equal(got[ma][:, :192], ref[ma][:, :192]) and torch.equal(got[mb][:, 192:], ref[mb][:, 192:]), (ra, rb)
        assert bool((got[~ma][:, :192] == SENTINEL).all()) and bool((got[~mb][:, 192:] == SENTINEL).all()), (ra, rb)
    got = run(RECTS[0], None)           # one layer restricted, the other on the whole map
    assert torch.equal(got[:, 192:], ref[:, 192:]) and bool((got[~_inside(RECTS[0])][:, :192] == SENTINEL).all())


def test_conv_1x1_pair(ops):
    """The streamed GEMM kernel: the wide 1x1 layer (convc1, 324 -> 256) and the flat 7x7 layer (convf1) alone and as a pair."""
    corr = ops.act_from_nchw(_rand(1, 324, H, W, seed=20), cs=352)
    flow = ops.act_from_nchw(_rand(1, 2, H, W, seed=21, scale=5.0), cs=4)
    c1 = _pc(ops, 256, 324, 1, 1, 22)
    f1 = ops.pack_conv(_rand(128, 2, 7, 7, seed=24, scale=0.1), _rand(128, seed=25, scale=0.1), flat_cs=4)

    def run(ra, rb, paired):
        a, b = (torch.full((H * W, n), SENTINEL, device="cuda") for n in (256, 128))
        pa = ops.conv_params(corr, c1, ops.Act(a, 1, H, W, 256), epi=1, precision="bf16x3")
        pb = ops.conv_params(flow, f1, ops.Act(b, 1, H, W, 128), epi=1, precision="bf16x3")
        assert pa.halo == pb.halo == 16 and ops.pair_ok(pa, pb)
        if ra:
            _set_roi(pa, ra)
        if rb:
            _set_roi(pb, rb)
        if paired:
            ops.run_conv_pair(pa, pb)
        else:
            ops.run_conv(pa)
            ops.run_conv(pb)
        torch.cuda.synchronize()
        return a, b

    ref = run(None, None, False)
    wide = (3, 0, 2, W)                 # (a rectangle of full width: runs that end at the right border)
    for paired in (False, True):
        for ra, rb in zip(RECTS + [wide], RECTS[2:] + RECTS[:2] + [wide]):
            got = run(ra, rb, paired)
            for g, r, rect in zip(got, ref, (ra, rb)):
                m = _inside(rect)
                assert torch.equal(g[m], r[m]), (paired, rect)
                assert bool((g[~m] == SENTINEL).all()), (paired, rect)


def test_unsupported_rectangles_are_refused(ops):
    """A kernel without rectangle support, or a rectangle outside the map, is WOFT_EINVAL -- never a silent whole-map launch."""
    from woft_amd._lib import WoftHipError
    x = ops.act_from_nchw(_rand(1, 64, H, W, seed=30))
    pc = _pc(ops, 128, 64, 3, 3, 31)
    mk = lambda: ops.Act(torch.full((H * W, 128), SENTINEL, device="cuda"), 1, H, W, 128)
    for halo, prec in ((0, "bf16x3"), (1, "bf16x3"), (4, "bf16x3"), (0, "fp32")):
        out = mk()
        p = ops.conv_params(x, pc, out, epi=1, precision=prec, halo=halo)
        assert p.halo == halo
        _set_roi(p, (5, 7, 9, 18))
        with pytest.raises(WoftHipError):
            ops.run_conv(p)
        torch.cuda.synchronize()
        assert bool((out.t == SENTINEL).all()), (halo, prec)
    for bad in ((-1, 0, 5, 5), (0, -1, 5, 5), (30, 0, 8, 5), (0, 50, 5, 4), (5, 5, 0, 4), (5, 5, 4, 0), (0, 0, H + 1, W), (5, 5, -2, 4)):
        out = mk()
        p = ops.conv_params(x, pc, out, epi=1, precision="bf16x3", halo=8)
        _set_roi(p, bad)
        with pytest.raises(WoftHipError):
            ops.run_conv(p)
        torch.cuda.synchronize()
        assert bool((out.t == SENTINEL).all()), bad


def test_lookup_regions_with_folded_gather(ops):
    """The volume-free lookup with the flow-head gather folded in: only the 8x8 blocks that intersect roi_* run (coordinate update
    of all their pixels), of those only the blocks that intersect smp_* write samples; everything bit-identical to the whole-map
    launch, everything else untouched."""
    from woft_amd._lib import WoftHipError
    from oracle import raft_ref
    c = 256
    f1, f2 = _rand(1, c, H, W, seed=40), _rand(1, c, H, W, seed=41)
    start = (raft_ref.coords_grid(1, H, W) + _rand(1, 2, H, W, seed=42, scale=3.0))[0].permute(1, 2, 0).reshape(H * W, 2).contiguous().cuda()
    a1, a2 = ops.act_from_nchw(f1), ops.act_from_nchw(f2)

    def split(t):
        o = torch.zeros(t.shape[0], 2 * c, dtype=torch.bfloat16, device="cuda")
        ops.split_bf16_lines(t, o)
        return o
    f2s, dims, cur = [], [], a2
    for l in range(4):
        f2s.append(split(cur.t))
        dims.append((cur.h, cur.w))
        if l < 3:
            nxt = ops.new_act(1, cur.h // 2, cur.w // 2, c)
            ops.avgpool2(cur, nxt)
            cur = nxt
    f1s = split(a1.t)
    n_planes = 2
    part = _rand(n_planes * H * W, 20, seed=43, scale=0.3).cuda()
    bias2 = _rand(2, seed=44, scale=0.1).cuda()

    def run(roi, smp):
        coords = start.clone()
        out = torch.full((H * W, 352), SENTINEL, device="cuda")
        delta, flow4, cat = (torch.full((H * W, n), SENTINEL, device="cuda") for n in (4, 4, 8))
        p = ops.make_lookup_otf_params(f1s, f2s, dims, H, W, c, coords, out, 4, 3)
        p.fh_part, p.fh_bias, p.fh_delta, p.fh_flow4, p.fh_flow_cat = (t.data_ptr() for t in (part, bias2, delta, flow4, cat))
        p.fh_planes, p.fh_ld, p.fh_ld_delta, p.fh_ld_cat = n_planes, 20, 4, 8
        if roi:
            p.roi_y0, p.roi_x0, p.roi_h, p.roi_w = roi
        if smp:
            p.smp_y0, p.smp_x0, p.smp_h, p.smp_w = smp
        ops.run_lookup_otf(p)
        torch.cuda.synchronize()
        return coords, out, delta, flow4, cat

    def blocks(rect):                   # pixels of the 8x8 blocks that intersect rect
        m = torch.zeros(H, W, dtype=torch.bool)
        m[rect[0] // 8 * 8:(rect[0] + rect[2] - 1) // 8 * 8 + 8, rect[1] // 8 * 8:(rect[1] + rect[3] - 1) // 8 * 8 + 8] = True
        return m.reshape(-1).cuda()

    ref = run(None, None)
    assert not bool((ref[1][:, :324] == SENTINEL).any()) and not torch.equal(ref[0], start)
    cases = [((2, 4, 15, 24), (5, 7, 9, 18)), ((20, 30, 1, 1), (20, 30, 1, 1)), ((0, 10, 9, 26), (0, 13, 6, 20)),
             ((27, 7, 10, 26), (30, 10, 7, 20)), ((7, 0, 15, 14), (10, 0, 9, 11)), ((26, 33, 11, 20), (29, 36, 8, 17)),
             ((0, 0, H, W), (12, 20, 3, 3)), ((0, 0, H, W), (0, 0, H, W)), ((5, 7, 9, 18), None)]
    for roi, smp in cases:
        got = run(roi, smp)
        mr, ms = blocks(roi), blocks(smp or roi)
        for k in (0, 2, 3, 4):          # coordinates, delta, flow4, the flow channels: the launched blocks, all their pixels
            cols = slice(0, 2)
            assert torch.equal(got[k][mr][:, cols], ref[k][mr][:, cols]), (roi, smp, k)
        assert torch.equal(got[0][~mr], start[~mr]), (roi, smp)
        for k in (2, 3, 4):
            assert bool((got[k][~mr] == SENTINEL).all()), (roi, smp, k)
        assert torch.equal(got[1][ms][:, :324], ref[1][ms][:, :324]), (roi, smp)
        assert bool((got[1][~ms] == SENTINEL).all()), (roi, smp)
    for bad in ((0, 0, H + 1, W), (-1, 0, 4, 4), (4, 4, 0, 4), (30, 50, 4, 4)):
        for which in ("roi", "smp"):
            coords = start.clone()
            out = torch.full((H * W, 352), SENTINEL, device="cuda")
            p = ops.make_lookup_otf_params(f1s, f2s, dims, H, W, c, coords, out, 4, 3)
            for f, v in zip(("y0", "x0", "h", "w"), bad):
                setattr(p, f"{which}_{f}", v)
            with pytest.raises(WoftHipError):
                ops.run_lookup_otf(p)
            torch.cuda.synchronize()
            assert bool((out == SENTINEL).all())
