"""The rectangle form of the chained fold on the host: the window rule chain_rect, the two new entry points in
the header, EXPORTS and the library, their argument checks (-1 before any device work), and the exactness argument -- the fp32
restatement on rectangles equals the fp32 full-frame restatement byte for byte wherever the chain stays inside the step rectangle,
and is invalid everywhere else."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import multiflow_host as MH
import multiflow_window_host as WH

ROOT = Path(__file__).resolve().parent.parent
NAN, INF = float("nan"), float("inf")


# ---- the window rule ------------------------------------------------------------------------------------------------------------
def _boxes():
    from woft_amd.window import Box
    rs = np.random.RandomState(5)
    for _ in range(300):
        W, H = int(rs.randint(64, 700)), int(rs.randint(64, 500))
        w, h = int(rs.randint(1, W)), int(rs.randint(1, H))
        x, y = int(rs.randint(0, W - w + 1)), int(rs.randint(0, H - h + 1))
        yield Box(x, y, w, h), float(rs.choice([0.1, 0.25, 0.5, 1.0])), W, H, int(rs.choice([8, 16, 32, 64])), int(rs.choice([16, 32, 160]))


def test_chain_rect_quantised_inside_the_frame_and_around_the_search_box():
    from woft_amd.window import chain_rect, search_box
    moved = 0
    for box, margin, W, H, q, m in _boxes():
        y0, x0, rows, cols = chain_rect(box, margin, W, H, q, m)
        sy0, sx0, srows, scols = search_box(box, margin, W, H, m).crop_rect()
        for o, n, side, so, sn in ((y0, rows, H, sy0, srows), (x0, cols, W, sx0, scols)):
            assert (n % q == 0 and n < side) or (o == 0 and n == side), (box, margin, W, H, q, m)
            assert 0 <= o and o + n <= side and n >= 1
            assert o <= so and so + sn <= o + n                               # (contains the search box's crop)
            if n < side and 0 < o < side - n:                                 # (not clamped: centred, the odd pixel after)
                assert o == so - (n - sn) // 2
                moved += 1
    assert moved > 50


def test_chain_rect_centring_and_both_clamps_by_hand():
    from woft_amd.window import Box, chain_rect, search_box
    # a 40 x 40 box in the middle: margins 10 -> 60 x 60 box -> crop 59 x 59 at (70, 90) -> 64 x 64, grown by 5: 2 before, 3 after
    box = Box(100, 80, 40, 40)
    assert search_box(box, 0.25, 640, 480, 32).crop_rect() == (70, 90, 59, 59)
    assert chain_rect(box, 0.25, 640, 480, 64, 32) == (68, 88, 64, 64)
    assert chain_rect(box, 0.25, 640, 480, 16, 32) == (68, 88, 64, 64)
    assert chain_rect(box, 0.25, 640, 480, 8, 32) == (68, 88, 64, 64)
    # at the frame's origin the growth is pushed inside (low clamp), at its far corner as well (high clamp)
    assert chain_rect(Box(0, 0, 40, 40), 0.25, 640, 480, 64, 32) == (0, 0, 64, 64)
    y0, x0, rows, cols = chain_rect(Box(600, 440, 40, 40), 0.25, 640, 480, 64, 32)
    assert (rows, cols) == (64, 64) and (y0 + rows, x0 + cols) == (480, 640)
    # a side whose multiple reaches the frame's: the whole side, the other axis still quantised
    assert chain_rect(Box(10, 80, 600, 40), 0.25, 640, 480, 64, 32) == (68, 0, 64, 640)
    # a falsy margin: the whole frame, every row and column (not the search box's crop, which drops one of each)
    for margin in (None, 0, 0.0, False):
        assert chain_rect(box, margin, 640, 480) == (0, 0, 480, 640)
    assert search_box(box, None, 640, 480).crop_rect() == (0, 0, 479, 639)
    # the default minimum size is the window tracker's
    assert chain_rect(box, 0.25, 640, 480) == (4, 24, 192, 192)


@pytest.mark.parametrize("quantum", [0, -8, 4, 12, 63, 8.0, "8", None, True])
def test_chain_rect_refuses_a_bad_quantum(quantum):
    from woft_amd.window import Box, chain_rect
    with pytest.raises(ValueError, match="quantum"):
        chain_rect(Box(10, 10, 20, 20), 0.25, 640, 480, quantum)
    with pytest.raises(ValueError, match="quantum"):
        chain_rect(Box(10, 10, 20, 20), None, 640, 480, quantum)              # (also where the margin would not use it)


# ---- the entry points -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from woft_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_header_exports_and_library_agree_on_the_new_names(lib):
    from woft_amd import _lib
    header = (ROOT / "include" / "woft_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(woft_\w+)\s*\(", header, flags=re.M))
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, n_args in (("woft_flow_chain_fold_window", 24), ("woft_chain_tc_window", 19)):
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name)
        assert len(_lib._SIGS[name][1]) == n_args
    assert lib.woft_abi_version() == raw.woft_abi_version()


def test_lazy_exports():
    import woft_amd
    from woft_amd import chained_window
    for name in ("chain_fold_window", "WindowedMultiFlowTracker", "WOFTChainedWindow"):
        assert getattr(woft_amd, name) is getattr(chained_window, name)


H9 = ctypes.c_double * 9


def test_fold_window_rejects_bad_arguments_without_a_device(lib):
    """-1 before any launch (host buffers stand in for device ones: nothing is dereferenced).  Every plane of the base call is a
    buffer of its own, so each case has exactly one thing wrong."""
    th, tw, sh, sw = 5, 7, 4, 9
    buf = (ctypes.c_float * 8192)()
    base = ctypes.addressof(buf)
    at = lambda j: base + 4 * 512 * j                         # (2 KiB apart: the largest plane pair is 288 B)
    eye = H9(1, 0, 0, 0, 1, 0, 0, 0, 1)
    good = dict(prev_flow=at(0), prev_cost=at(1), prev_vis=at(2), th=th, tw=tw, ty0=3, tx0=2, step_flow=at(3), step_wlogit=at(4),
                step_mlogit=at(5), sh=sh, sw=sw, sy0=1, sx0=6, post_H=None, unit_cost=1.0, vis_thr=0.5, k=3, first=0,
                best_flow=at(6), best_cost=at(7), best_vis=at(8), best_sel=at(9))
    order = list(good)

    def fold(**kw):
        d = dict(good, **kw)
        return lib.woft_flow_chain_fold_window(*[d[n] for n in order], None)

    tp, sp = 4 * th * tw, 4 * sh * sw
    top = 1 << 24
    bad = [dict(step_flow=None), dict(best_flow=None), dict(best_cost=None), dict(best_vis=None), dict(best_sel=None),
           # a partly-null prev triple: every mix but all / none
           dict(prev_flow=None), dict(prev_cost=None), dict(prev_vis=None), dict(prev_flow=None, prev_cost=None),
           dict(prev_flow=None, prev_vis=None), dict(prev_cost=None, prev_vis=None),
           # aliasing: the running best shares bytes with an input, or with itself (each plane with its own size)
           dict(best_cost=good["prev_cost"]), dict(best_vis=good["prev_vis"]), dict(best_flow=good["prev_flow"]),
           dict(best_flow=good["step_flow"]), dict(best_flow=good["step_flow"] + sp), dict(best_flow=good["step_flow"] - tp),
           dict(best_cost=good["step_flow"] + 2 * sp - 4), dict(best_sel=good["step_mlogit"]), dict(best_vis=good["step_wlogit"]),
           dict(best_vis=good["step_wlogit"] + sp - 4), dict(best_sel=good["prev_flow"] + tp), dict(best_vis=good["best_cost"]),
           dict(best_cost=good["best_flow"] + tp), dict(best_sel=good["best_vis"] + 4),
           dict(prev_flow=None, prev_cost=None, prev_vis=None, best_flow=good["step_flow"]),
           # a non-positive side, a negative origin, origin + side beyond 2^24
           dict(th=0), dict(tw=0), dict(sh=0), dict(sw=0), dict(th=-1), dict(tw=-5), dict(sh=-2), dict(sw=-1),
           dict(ty0=-1), dict(tx0=-1), dict(sy0=-1), dict(sx0=-3),
           dict(ty0=top - th + 1), dict(tx0=top - tw + 1), dict(sy0=top - sh + 1), dict(sx0=top - sw + 1), dict(tx0=(1 << 31) - 1),
           # k, unit_cost, vis_thr
           dict(k=-1), dict(k=128), dict(k=1 << 20), dict(unit_cost=NAN), dict(unit_cost=-0.5), dict(unit_cost=-INF),
           dict(vis_thr=-0.01), dict(vis_thr=1.01), dict(vis_thr=NAN), dict(vis_thr=INF),
           # post_H: not finite, or not normalised
           dict(post_H=H9(1, 0, 0, 0, 1, 0, 0, 0, 2)), dict(post_H=H9(1, 0, 0, 0, 1, 0, 0, 0, 0)),
           dict(post_H=H9(1, 0, 0, 0, 1, 0, 0, 0, -1)), dict(post_H=H9(1, 0, NAN, 0, 1, 0, 0, 0, 1)),
           dict(post_H=H9(INF, 0, 0, 0, 1, 0, 0, 0, 1)), dict(post_H=H9(1, 0, 0, 0, 1, 0, 0, -INF, 1)),
           dict(post_H=H9(1, 0, 0, 0, 1, 0, 0, 0, NAN))]
    for kw in bad:
        assert fold(**kw) == -1, kw
    # (with a post_H every other check still stands)
    assert fold(post_H=eye, k=128) == -1 and fold(post_H=eye, best_cost=good["prev_cost"]) == -1


def test_chain_tc_window_rejects_bad_arguments_without_a_device(lib):
    gh, gw = 5, 7
    buf = (ctypes.c_float * 8192)()
    base = ctypes.addressof(buf)
    at = lambda j: base + 4 * 512 * j
    good = dict(flow=at(0), cost=at(1), vis=at(2), sel=at(3), tmask=at(4), gh=gh, gw=gw, mh=gh + 1, mw=gw + 2, ty0=3, tx0=2,
                frame_h=40, frame_w=50, vis_thr=0.5, dst=at(5), w=at(6), ok=at(7), hist=at(8))
    order = list(good)

    def tc(**kw):
        d = dict(good, **kw)
        return lib.woft_chain_tc_window(*[d[n] for n in order], None)

    plane, top = 4 * gh * gw, 1 << 24
    bad = [dict(flow=None), dict(cost=None), dict(vis=None), dict(sel=None), dict(dst=None), dict(ok=None),
           dict(gh=0), dict(gw=0), dict(gh=-1), dict(gw=top + 1), dict(mh=gh - 1), dict(mw=gw - 1),
           dict(vis_thr=-0.01), dict(vis_thr=1.01), dict(vis_thr=NAN),
           dict(dst=good["flow"]), dict(dst=good["flow"] + plane), dict(w=good["cost"]), dict(ok=good["vis"]), dict(hist=good["sel"]),
           dict(ok=good["tmask"]), dict(w=good["dst"] + plane), dict(ok=good["w"]), dict(hist=good["ok"] + 4),
           # the rectangle and the frame
           dict(ty0=-1), dict(tx0=-1), dict(ty0=top - gh + 1), dict(tx0=top - gw + 1),
           dict(frame_h=0), dict(frame_w=0), dict(frame_h=-4), dict(frame_w=top + 1)]
    for kw in bad:
        assert tc(**kw) == -1, kw


def test_python_layers_reject_bad_arguments_before_any_device_work():
    import torch
    from woft_amd import chain_fold_window
    f = torch.zeros(2, 4, 4)
    R = (0, 0, 4, 4)
    for kw, match in ((dict(k=-1), "k must"), (dict(k=128), "k must"), (dict(k=0, vis_thr=1.5), "vis_thr"),
                      (dict(k=0, unit_cost=-1.0), "unit_cost")):
        with pytest.raises(ValueError, match=match):
            chain_fold_window(None, None, (f,), template_rect=R, step_rect=R, **kw)
    for rects, match in ((dict(template_rect=(0, 0, 0, 4), step_rect=R), "template_rect"),
                         (dict(template_rect=R, step_rect=(-1, 0, 4, 4)), "step_rect"),
                         (dict(template_rect=R, step_rect=(0, 0, 4)), "step_rect"),
                         (dict(template_rect=R, step_rect=(0, 0, 4, 5)), r"\(2, 4, 5\)")):
        with pytest.raises(ValueError, match=match):
            chain_fold_window(None, None, (f,), 0, **rects)


# ---- exactness of the window form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,trect,srect", WH.RECT_CASES)
def test_window_restatement_is_the_full_frame_one_inside_the_step_rect_and_invalid_outside(case, trect, srect):
    """fp32 against fp32: the candidate on rectangles has the bytes of the full-frame candidate at every template-rect pixel whose q
    lies in the step rect (u = q - origin is exact there, the taps are the same numbers), and is invalid at every other pixel."""
    h, w, K = case
    n_in = n_all = 0
    for prev, step in MH.make_case(h, w, K):
        ok_f, flow_f, cost_f, vis_f = MH.candidate(prev, step, 1.0, np.float32)
        ok_w, flow_w, cost_w, vis_w = WH.candidate(*WH.crop_case(prev, step, trect, srect), trect, srect, 1.0, np.float32)
        ys, xs = np.mgrid[trect[0]:trect[0] + trect[2], trect[1]:trect[1] + trect[3]]
        pf = WH.crop(prev[0], trect)
        qx, qy = (xs.astype(np.float32) + pf[0]).astype(np.float32), (ys.astype(np.float32) + pf[1]).astype(np.float32)
        inside = ((qx >= srect[1]) & (qx <= srect[1] + srect[3] - 1) & (qy >= srect[0]) & (qy <= srect[0] + srect[2] - 1))
        assert np.array_equal(ok_w, inside) and WH.crop(ok_f, trect)[inside].all()
        for a, b in ((flow_f, flow_w), (cost_f, cost_w), (vis_f, vis_w)):
            assert a.dtype == b.dtype == np.float32
            assert np.array_equal(WH.crop(a, trect)[..., inside].view(np.uint32), b[..., inside].view(np.uint32))
        n_in, n_all = n_in + int(inside.sum()), n_all + inside.size
    assert 0.25 <= n_in / n_all <= 0.75, n_in / n_all                         # (both branches are exercised)


@pytest.mark.parametrize("case", MH.CASES)
def test_window_restatement_at_zero_origins_is_the_full_frame_one(case):
    h, w, K = case
    cands = MH.make_case(h, w, K)
    R = (0, 0, h, w)
    for dtype in (np.float32, np.float64):
        a, ma = MH.fold_all(cands, dtype=dtype)
        b, mb = WH.fold_all(cands, R, [R] * K, dtype=dtype)
        assert all(np.array_equal(a[n], b[n], equal_nan=True) for n in a) and ma == mb


def test_post_H_restatement_by_hand():
    """A zero flow on a 3 x 4 rectangle at (10, 20) through a translation by (2, -1): flow (2, -1) everywhere; through a matrix whose
    denominator is 1 - x / 21.5: invalid in the columns x = 22 and 23."""
    trect = (10, 20, 3, 4)
    step = (np.zeros((2, 3, 4), np.float32), None, None)
    T = np.array([[1, 0, 2], [0, 1, -1], [0, 0, 1.0]])
    for dtype in (np.float32, np.float64):
        b = WH.fold(None, None, step, 0, trect, trect, dtype=dtype, post_H=T)
        assert (b["sel"] == 0).all() and (b["flow"][0] == 2).all() and (b["flow"][1] == -1).all()
        V = np.array([[1, 0, 0], [0, 1, 0], [-1 / 21.5, 0, 1.0]])
        b = WH.fold(None, None, step, 0, trect, trect, dtype=dtype, post_H=V)
        den = WH.post_den(None, step, trect, trect, V)
        assert np.array_equal(b["sel"] >= 0, den > 0) and (b["sel"][:, :2] == 0).all() and (b["sel"][:, 2:] == -1).all()
        assert np.isnan(b["flow"][:, den <= 0]).all()
        # x = 20 maps to 20 / (1 - 20 / 21.5): a flow of 20 * 21.5 / 1.5 - 20
        assert np.allclose(b["flow"][0, :, 0], 20 * 21.5 / 1.5 - 20, rtol=1e-6, atol=0)
