"""The rectangle form of the chained fold on the GPU: woft_flow_chain_fold_window against woft_flow_chain_fold
(bytes: at zero origins everywhere, on rectangles wherever the chain stays inside the step rectangle) and against the float64
restatement (tests/multiflow_window_host.py) under section 18's rule -- 4 x the float32 restatement's own error, 1e-6 floor --,
the window's edges, planted non-finite values, the closing homography, and woft_chain_tc_window against woft_chain_tc plus the
in-frame rule evaluated in numpy fp32.

Measured on the MI355X (`pytest -s` prints them): (a) = the smallest cost margin, (b) = the smallest visibility margin of the
float64 restatement; then max |got - ref64| / its bound.  Both fold orders give the same figures to the digits shown.

    case                     (a)     (b)     flow              cost              vis
    37 x 131, K=7, rects     0.4405  0.1614  3.3e-07 / 4.7e-06 1.3e-07 / 3.1e-06 9.2e-08 / 9.6e-07
    9 x 70, K=3, rects       0.4422  0.1633  3.0e-07 / 4.5e-06 6.3e-08 / 1.1e-06 1.1e-07 / 9.5e-07
    64 x 96, K=3, rects      0.4379  0.1596  3.1e-07 / 4.3e-06 7.2e-08 / 1.1e-06 1.1e-07 / 9.6e-07
    post_H identity          -       -       3.2e-07 / 4.5e-06
    post_H general           -       -       4.4e-07 / 7.2e-06
    post_H vanishing line    invalid share 0.485, min |den| 2.55e-03: 9.6e-04 / 9.8e-03 (flows up to 1e4 px next to the line)
    chain_tc_window          0.339 (origin 0) and 0.287 (origin (3, 5)) of the gated landings leave the frame
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import multiflow_host as MH  # noqa: E402
import multiflow_window_host as WH  # noqa: E402
from woft_amd import ops  # noqa: E402

NAN, INF = float("nan"), float("inf")
THR = 0.5
FIELDS = ("flow", "cost", "vis")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(best):
    return dict(zip(("flow", "cost", "vis", "sel"), (t.cpu().numpy() for t in best)))


def full_fold(best, prev, step, k):
    prev = None if prev is None else tuple(cuda(p) for p in prev)
    return ops.flow_chain_fold(best, prev, cuda(step[0]), cuda(step[1]), cuda(step[2]), k=k, vis_thr=THR, first=best is None)


def win_fold(best, prev, step, k, trect, srect, post_H=None):
    """One woft_flow_chain_fold_window launch on numpy planes already cut to the rectangles."""
    prev = None if prev is None else tuple(cuda(p) for p in prev)
    step = tuple(step) + (None,) * (3 - len(step))
    return ops.flow_chain_fold_window(best, prev, cuda(step[0]), cuda(step[1]), cuda(step[2]), k=k, template_rect=trect,
                                      step_rect=srect, post_H=post_H, vis_thr=THR, first=best is None)


def same_bits(a, b, where=None):
    where = np.ones(a["sel"].shape, bool) if where is None else where
    return all(np.array_equal(bits(a[n][..., where]), bits(b[n][..., where])) for n in FIELDS) \
        and np.array_equal(a["sel"][where], b["sel"][where])


def is_empty(got, where):
    return (np.isnan(got["flow"][:, where]).all() and np.isposinf(got["cost"][where]).all() and not got["vis"][where].any()
            and (got["sel"][where] == -1).all())


def check_against_restatement(got, ref64, ref32, tag):
    """sel and the empty pixels at EVERY pixel; on the others max |got - ref64| <= max(4 * max |ref32 - ref64|, 1e-6 * max |ref64|)."""
    assert np.array_equal(got["sel"], ref64["sel"]), f"{tag}: {(got['sel'] != ref64['sel']).sum()} pixels select another candidate"
    fin = ref64["sel"] >= 0
    assert fin.any() and is_empty(got, ~fin) and not np.isnan(got["flow"][:, fin]).any()
    for n in FIELDS:
        r64, r32, g = ref64[n][..., fin], ref32[n][..., fin].astype(np.float64), got[n][..., fin].astype(np.float64)
        bound = max(4 * np.abs(r32 - r64).max(), 1e-6 * np.abs(r64).max())
        diff = np.abs(g - r64).max()
        print(f"{tag}: {n} max |got - ref64| {diff:.1e} / {bound:.1e}")
        assert diff <= bound, f"{tag}: {n} max |got - ref64| {diff:.3e} > {bound:.3e}"


# ---- 1. zero origins: the bytes of woft_flow_chain_fold -------------------------------------------------------------------------
@pytest.mark.parametrize("case", MH.CASES)
def test_zero_origins_give_the_full_frame_kernels_bytes(case):
    h, w, K = case
    R = (0, 0, h, w)
    a = b = None
    for k, (prev, step) in enumerate(MH.make_case(h, w, K)):
        a, b = full_fold(a, prev, step, k), win_fold(b, prev, step, k, R, R)
    a, b = host(a), host(b)
    assert same_bits(a, b) and (a["sel"] >= 0).any() and (a["sel"] < 0).any()
    # ... and with a null prev
    prev, step = MH.make_case(h, w, K)[0]
    assert same_bits(host(full_fold(None, None, step, 2)), host(win_fold(None, None, step, 2, R, R)))


# ---- 2. rectangles --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rect_cases():
    """Per rectangle pair: the full-frame candidates, one step rectangle per candidate (the pair's, shifted), the candidates cut to
    the rectangles, and the float64 / float32 restatements of both fold orders (computed once, left unchanged)."""
    out = {}
    for case, trect, srect in WH.RECT_CASES:
        h, w, K = case
        full = MH.make_case(h, w, K)
        srects = [(srect[0] + k % 3 - 1, srect[1] + 2 * (k % 2), srect[2], srect[3]) for k in range(K)]
        assert all(0 <= r[0] and r[0] + r[2] <= h and 0 <= r[1] and r[1] + r[3] <= w for r in srects) and len(set(srects)) >= 2
        cut = [WH.crop_case(p, s, trect, r) for (p, s), r in zip(full, srects)]
        orders = {o: (WH.fold_all(cut, trect, srects, THR, order=o), WH.fold_all(cut, trect, srects, THR, dtype=np.float32, order=o)[0])
                  for o in (tuple(range(K)), tuple(reversed(range(K))))}
        out[case] = dict(full=full, trect=trect, srect=srect, srects=srects, cut=cut, orders=orders)
    return out


@pytest.mark.parametrize("case", [c for c, _, _ in WH.RECT_CASES])
def test_single_candidate_is_the_full_frame_kernels_crop_inside_and_empty_outside(rect_cases, case):
    c = rect_cases[case]
    trect, srect = c["trect"], c["srect"]
    n_in = n_all = 0
    for k, (prev, step) in enumerate(c["full"]):
        want = {n: WH.crop(v, trect) for n, v in host(full_fold(None, prev, step, k)).items()}
        got = host(win_fold(None, *WH.crop_case(prev, step, trect, srect), k, trect, srect))
        _, u = WH.landing(WH.crop(prev[0], trect), trect, srect)
        inside = (u[0] >= 0) & (u[0] <= srect[3] - 1) & (u[1] >= 0) & (u[1] <= srect[2] - 1)
        assert same_bits(got, want, inside) and (got["sel"][inside] == k).all() and is_empty(got, ~inside)
        n_in, n_all = n_in + int(inside.sum()), n_all + inside.size
    assert 0.25 <= n_in / n_all <= 0.75


@pytest.mark.parametrize("case", [c for c, _, _ in WH.RECT_CASES])
def test_k_candidates_with_a_step_rect_each_against_the_restatement(rect_cases, case):
    c = rect_cases[case]
    for order, ((ref64, margins), ref32) in c["orders"].items():
        a, b = margins["cost"], margins["vis"]
        print(f"{case} order {order}: (a) smallest cost margin {a:.4f}, (b) smallest visibility margin {b:.4f}")
        assert a >= 1e-3 and b >= 1e-3
        best = None
        for k in order:
            best = win_fold(best, *c["cut"][k], k, c["trect"], c["srects"][k])
        got = host(best)
        assert len(set(np.unique(got["sel"]).tolist()) - {-1}) >= 2
        check_against_restatement(got, ref64, ref32, f"{case} order {order[0]}..")


# ---- 3. the window's edges ------------------------------------------------------------------------------------------------------
def test_last_row_and_column_are_valid_half_a_pixel_outside_is_not():
    trect, srect = (2, 3, 5, 6), (1, 2, 6, 8)
    (ty0, tx0, th, tw), (sy0, sx0, sh, sw) = trect, srect
    ys, xs = np.mgrid[ty0:ty0 + th, tx0:tx0 + tw].astype(np.float32)
    # where every pixel of a template row lands, in frame coordinates: (x, y, valid, the step pixel whose data comes back)
    last_x, last_y = sx0 + sw - 1, sy0 + sh - 1
    rows = [(last_x, sy0 + 2, True, (2, sw - 1)), (sx0 + 3, last_y, True, (sh - 1, 3)), (last_x, last_y, True, (sh - 1, sw - 1)),
            (last_x + 0.5, sy0 + 2, False, None), (sx0 + 3, last_y + 0.5, False, None)]
    target = np.zeros((2, th, tw), np.float32)
    for y, (qx, qy, _, _) in enumerate(rows):
        target[0, y], target[1, y] = qx, qy
    target[0, 3, 1], target[1, 4, 1] = sx0 - 0.5, sy0 - 0.5                   # (... and half a pixel before the first column / row)
    target[1, 4, 2], target[0, 4, 2] = sy0, sx0                                # (the first row and column: valid)
    pflow = target - np.stack([xs, ys])
    one = np.ones((th, tw), np.float32)
    sflow = np.stack([np.arange(sh * sw, dtype=np.float32).reshape(sh, sw), -np.arange(sh * sw, dtype=np.float32).reshape(sh, sw)])
    got = host(win_fold(None, (pflow, 0 * one, one), (sflow,), 0, trect, srect))
    want_valid = np.array([[ok] * tw for _, _, ok, _ in rows])
    want_valid[3, 1] = want_valid[4, 1] = False
    want_valid[4, 2] = True
    assert np.array_equal(got["sel"] >= 0, want_valid) and is_empty(got, ~want_valid)
    for y, (_, _, ok, at) in enumerate(rows):
        if ok:
            v = sflow[0][at]
            assert (got["flow"][0, y] == pflow[0, y] + v).all() and (got["flow"][1, y] == pflow[1, y] - v).all()
    assert got["flow"][0, 4, 2] == pflow[0, 4, 2] + sflow[0, 0, 0]


# ---- 4. planted non-finite values -----------------------------------------------------------------------------------------------
def test_planted_non_finite_step_values_invalidate_exactly_the_pixels_whose_taps_touch_them(rect_cases):
    c = rect_cases[(37, 131, 7)]
    trect, srect = c["trect"], c["srect"]
    prev, step = WH.crop_case(*c["full"][0], trect, srect)
    _, u = WH.landing(prev[0], trect, srect)
    t = WH.taps(u[0], u[1], srect[2], srect[3])
    planted = [s.copy() for s in step]
    affected = np.zeros(t["valid"].shape, bool)
    for plane, idx, v in ((0, (0, 3, 7), NAN), (0, (1, 9, 20), INF), (0, (0, 12, 28), -INF), (1, (5, 12), NAN), (1, (7, 25), INF),
                          (1, (14, 5), -INF), (2, (2, 16), NAN), (2, (10, 10), INF), (2, (13, 30), -INF)):
        planted[plane][idx] = v
        j = idx[-2] * srect[3] + idx[-1]
        # (a zero weight on an infinity is a NaN: every pixel one of whose four taps is the planted one; found from clean fields)
        affected |= t["valid"] & ((t["i00"] == j) | (t["i01"] == j) | (t["i10"] == j) | (t["i11"] == j))
    clean, got = host(win_fold(None, prev, step, 0, trect, srect)), host(win_fold(None, prev, planted, 0, trect, srect))
    assert affected.sum() >= 9 and (clean["sel"][affected] == 0).all()
    assert is_empty(got, affected) and same_bits(got, clean, ~affected)
    # folded second: the affected pixels keep the earlier best
    first = win_fold(None, *c["cut"][1], 1, trect, c["srects"][1])
    before = host(tuple(x.clone() for x in first))
    got = host(win_fold(first, prev, planted, 0, trect, srect))
    clean = host(win_fold(win_fold(None, *c["cut"][1], 1, trect, c["srects"][1]), prev, step, 0, trect, srect))
    assert same_bits(got, before, affected) and same_bits(got, clean, ~affected) and (clean["sel"][affected] == 0).any()


# ---- 5. the closing homography --------------------------------------------------------------------------------------------------
GENERAL_H = np.array([[1.01, 0.02, 1.5], [-0.015, 0.99, -2.0], [1e-4, -2e-4, 1.0]])
VANISHING_H = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1 / 24.0, 0.004, 1.0]])     # den = 0 on a line that crosses the rectangle


@pytest.mark.parametrize("name", ["identity", "general", "vanishing"])
def test_post_H_against_the_restatement(rect_cases, name):
    c = rect_cases[(37, 131, 7)]
    trect, srect = c["trect"], c["srect"]
    prev, step = WH.crop_case(*c["full"][0], trect, srect)
    Hm = dict(identity=np.eye(3), general=GENERAL_H, vanishing=VANISHING_H)[name]
    den = WH.post_den(prev, step, trect, srect, Hm)
    tap_ok = np.isfinite(den)
    share = float((den[tap_ok] <= 0).mean())
    print(f"post_H {name}: invalid share {share:.3f}, min |den| {np.abs(den[tap_ok]).min():.2e}")
    assert np.abs(den[tap_ok]).min() >= 1e-3
    if name == "vanishing":
        assert 0.1 <= share <= 0.9
    else:
        assert share == 0
    ref64 = WH.fold(None, prev, step, 4, trect, srect, THR, post_H=Hm)
    ref32 = WH.fold(None, prev, step, 4, trect, srect, THR, dtype=np.float32, post_H=Hm)
    got = host(win_fold(None, prev, step, 4, trect, srect, post_H=Hm))
    assert np.array_equal(got["sel"] >= 0, tap_ok & (den > 0))                # (invalid exactly where den <= 0, or the tap is)
    check_against_restatement(got, ref64, ref32, f"post_H {name}")
    if name == "identity":                                                     # (H r = r: only the rounding of P + flow - P remains)
        plain = host(win_fold(None, prev, step, 4, trect, srect))
        assert np.array_equal(got["sel"], plain["sel"]) and np.array_equal(bits(got["cost"]), bits(plain["cost"]))
    # folded second, an invalid landing keeps the earlier best
    if name == "vanishing":
        first = win_fold(None, *c["cut"][1], 1, trect, c["srects"][1])
        before = host(tuple(x.clone() for x in first))
        got = host(win_fold(first, prev, step, 0, trect, srect, post_H=Hm))
        gone = tap_ok & (den <= 0)
        assert same_bits(got, before, gone) and (got["sel"] == 0).any()


def test_public_function_on_host_and_device_tensors(rect_cases):
    from woft_amd import chain_fold_window
    c = rect_cases[(9, 70, 3)]
    K = len(c["cut"])
    best = None
    for k in range(K):
        best = win_fold(best, *c["cut"][k], k, c["trect"], c["srects"][k])
    want = host(best)
    th, tw = c["trect"][2:]
    for dev in ("cpu", "cuda"):
        T = lambda a: torch.from_numpy(a).to(dev)
        best = None
        for k, (prev, step) in enumerate(c["cut"]):
            before = None if best is None else [b.clone() for b in best]
            new = chain_fold_window(best, tuple(T(p) for p in prev), tuple(T(s) for s in step), k, c["trect"], c["srects"][k])
            if before is not None:
                ib = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
                assert all(torch.equal(ib(a), ib(b)) for a, b in zip(best, before))        # (the caller's best is left alone)
            best = new
        assert all(b.device.type == dev for b in best) and [tuple(b.shape) for b in best] == [(2, th, tw)] + [(1, th, tw)] * 3
        got = dict(zip(("flow", "cost", "vis", "sel"), (b.cpu().numpy().reshape(-1, th, tw) for b in best)))
        assert np.array_equal(bits(got["flow"]), bits(want["flow"])) and np.array_equal(got["sel"][0], want["sel"])
        assert np.array_equal(bits(got["cost"][0]), bits(want["cost"])) and np.array_equal(bits(got["vis"][0]), bits(want["vis"]))


# ---- 6. chain_tc_window ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [(0, 0), (3, 5)])
@pytest.mark.parametrize("masked", [False, True])
def test_chain_tc_window_is_chain_tc_plus_the_in_frame_rule(origin, masked):
    h, w, K = 37, 131, 7
    best = None
    for k, (prev, step) in enumerate(MH.make_case(h, w, K)):
        best = full_fold(best, prev, step, k)
    flow, cost, vis, sel = best
    flow = (flow * 8).contiguous()                                             # (up to +-40 px: many landings leave the frame)
    ty0, tx0 = origin
    frame_hw = (ty0 + h + 2, tx0 + w + 4)
    rs = np.random.RandomState(3)
    mask_hw = (h + 1, w + 3)
    mask = cuda((rs.uniform(size=mask_hw) < 0.5).astype(np.uint8) * 255) if masked else None
    a = ops.chain_tc(flow, cost, vis, sel, mask, THR, mask_hw=mask_hw if masked else None)
    b = ops.chain_tc_window(flow, cost, vis, sel, mask, THR, origin, frame_hw, mask_hw=mask_hw if masked else None)
    for x, y in zip(a[:2], b[:2]):                                             # dst, w: the bytes, NaN included
        assert np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy()))
    assert torch.equal(a[3], b[3]) and int(a[3].sum()) == (h * w if not masked else int((mask[:h, :w] != 0).sum()))
    f = flow.cpu().numpy()
    ys, xs = np.mgrid[:h, :w]
    with np.errstate(invalid="ignore"):
        X = ((tx0 + xs).astype(np.float32) + f[0]).astype(np.float32)
        Y = ((ty0 + ys).astype(np.float32) + f[1]).astype(np.float32)
        out = (X < 0) | (Y < 0) | (np.rint(X) >= np.float32(frame_hw[1])) | (np.rint(Y) >= np.float32(frame_hw[0]))
    ok_tc = a[2].cpu().numpy().reshape(h, w)
    share = float(out[ok_tc > 0].mean())
    print(f"origin {origin}: {share:.3f} of the gated landings leave the {frame_hw} frame")
    assert 0.1 <= share <= 0.9
    want = np.where(out, np.float32(0), ok_tc).astype(np.float32)
    assert np.array_equal(bits(b[2].cpu().numpy().reshape(h, w)), bits(want))
    # no weights asked: none computed, the rest unchanged
    c = ops.chain_tc_window(flow, cost, vis, sel, mask, THR, origin, frame_hw, want_w=False, mask_hw=mask_hw if masked else None)
    assert c[1] is None and torch.equal(c[2], b[2]) and torch.equal(c[3], b[3])
