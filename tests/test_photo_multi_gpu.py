"""The multi-target photometric refinement on the device (woft_photo_eval_multi, woft_photo_refine_multi, PhotoTemplateMulti;
DESIGN.md section 29): K targets of one template and one frame must get, target by target, the bytes the single-target entry points
write -- the same chunks summed in the same order -- whatever the other targets do; one call and one read whatever K; and the
recorded iterates stay within the float32 yardstick of the float64 restatement.  Run with -s for the figures."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import chained_multi_util as U  # noqa: E402
import photo_host as ph  # noqa: E402
import photo_multi_host as pm  # noqa: E402
from woft_amd import _lib, ops, photo  # noqa: E402
from woft_amd.chained import pack_target_bits  # noqa: E402


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def scene():
    t, _, f, H_gt, W0 = ph.base_case(ph.SEEDS[0])
    rs = np.random.RandomState(5)
    return dict(t=t, f=f, H_gt=H_gt, W0=W0, t32=t.astype(np.float32) * np.float32(0.97) + np.float32(1.3),
                f32=f.astype(np.float32) + rs.uniform(-0.5, 0.5, f.shape).astype(np.float32),
                w=np.where(rs.uniform(size=t.shape[:2]) < 0.1, 0.0, rs.uniform(0.0, 2.0, t.shape[:2])).astype(np.float32))


# gain_bias, huber_k, stride, weights: each switched alone, then all together
OPTIONS = [dict(gain_bias=True, huber_k=None, stride=1, weights=False), dict(gain_bias=False, huber_k=None, stride=1, weights=False),
           dict(gain_bias=True, huber_k=6.0, stride=1, weights=False), dict(gain_bias=True, huber_k=None, stride=2, weights=False),
           dict(gain_bias=True, huber_k=None, stride=1, weights=True), dict(gain_bias=False, huber_k=4.0, stride=2, weights=True)]
DTYPES = {"u8/u8": ("t", "f"), "f32/u8": ("t32", "f"), "u8/f32": ("t", "f32")}


@pytest.mark.parametrize("K", [1, 3, 32])
@pytest.mark.parametrize("dtypes", sorted(DTYPES))
def test_bytes_of_the_single_path(scene, K, dtypes):
    tmpl, frame = (scene[k] for k in DTYPES[dtypes])
    masks, Ws = pm.mask_set(K), pm.poses(scene["W0"], K)
    bits = dev(pack_target_bits(masks).view(np.int32))
    d_t, d_f = dev(tmpl), dev(frame)
    statuses = set()
    for opt in OPTIONS:
        weights, stride, gb, hk = (scene["w"] if opt["weights"] else None), opt["stride"], opt["gain_bias"], opt["huber_k"]
        nu = 10 if gb else 8
        multi = photo.PhotoTemplateMulti(d_t, masks, stride=stride, weights=weights)
        singles = [photo.PhotoTemplate(d_t, m, stride=stride, weights=weights) for m in masks]
        for t, s in enumerate(singles):
            assert (multi.boxes[t], multi.n_sets[t]) == (s.box, s.n_set)
            if s.box is not None:
                assert (multi.centres[t], multi.scales[t]) == (s.centre, s.scale)
        # the accumulate kernel alone: row t of the batched evaluation is woft_photo_eval on mask t, untouched where inactive
        active = [int(s._launchable(nu)) for s in singles]
        out = torch.full((K, ops.PHOTO_NACC), float("nan"), dtype=torch.float64, device="cuda")
        gains, biases = [1.0 + 0.01 * t for t in range(K)], [-12.0 + t for t in range(K)]
        ops.photo_eval_multi(d_t, bits, multi.weights, d_f, multi._call_boxes, stride, Ws, gains, biases, active, gb, hk, out)
        out = out.cpu().numpy()
        for t, s in enumerate(singles):
            one = torch.full((ops.PHOTO_NACC,), float("nan"), dtype=torch.float64, device="cuda")
            if active[t]:
                ops.photo_eval(d_t, s.mask, s.weights, d_f, s.box, stride, Ws[t], gains[t], biases[t], gb, hk, one)
                assert np.isfinite(out[t, :nu * (nu + 1) // 2 + nu + 3]).all()
            assert out[t].tobytes() == one.cpu().numpy().tobytes(), (K, dtypes, opt, t)
        # whole refinements
        kw = dict(iters=5, gain_bias=gb, huber_k=hk)
        Hs, infos = multi.refine(d_f, Ws, **kw)
        assert Hs.shape == (K, 3, 3) and Hs.dtype == np.float64 and len(infos) == K
        for t, s in enumerate(singles):
            want = s.refine(d_f, Ws[t], **kw)
            pm.assert_same_refinement((Hs[t], infos[t]), want, (K, dtypes, opt, t))
            statuses.add(infos[t].status)
            if not active[t]:
                assert (infos[t].status, infos[t].best, len(infos[t].cost)) == ("TOO_FEW", -1, 0) and np.array_equal(Hs[t], Ws[t])
    print(f"K {K} {dtypes}: statuses seen {sorted(statuses)}")
    assert ops.photo_multi_partials(multi._call_boxes, 1) == 2                # (the base mask's box: two partials next to one)
    if K >= 3:
        assert ops.photo_multi_partials(multi._call_boxes[1:], 1) == 1 and "TOO_FEW" in statuses


def test_normal_equations_returns_k_tuples(scene):
    masks = pm.mask_set(3)[:2]
    Ws = pm.poses(scene["W0"], 2)
    got = photo.PhotoTemplateMulti(scene["t"], masks).normal_equations(scene["f"], Ws, gains=[1.05, 0.98], biases=[-4.0, 2.0], huber_k=6.0)
    assert len(got) == 2
    for t, (G, r, cost, n) in enumerate(got):
        G1, r1, cost1, n1 = photo.PhotoTemplate(scene["t"], masks[t]).normal_equations(scene["f"], Ws[t], gain=[1.05, 0.98][t],
                                                                                     bias=[-4.0, 2.0][t], huber_k=6.0)
        assert np.array_equal(G, G1) and np.array_equal(r, r1) and cost == cost1 and n == n1 and n > 0
    with pytest.raises(ValueError):
        photo.PhotoTemplateMulti(scene["t"], pm.mask_set(3)).normal_equations(scene["f"], pm.poses(scene["W0"], 3))


def test_targets_stop_independently(scene):
    """In one call: a target that converges early, one that runs to the last iterate, one that starts outside the frame (TOO_FEW at
    iterate 0) and an inactive one."""
    t, f, W0 = scene["t"], scene["f"], scene["W0"]
    base, other = pm.mask_set(3)[:2]
    masks = [base, other, pm.mask_set(32)[31], base]
    # (a near-exact pose of the first target: the last iterate of a converged run -- without gain and bias, whose restart at 1
    #  and 0 would be a step of its own)
    _, info = photo.refine_homography(t, base, f, W0, iters=20, eps=1e-7, gain_bias=False)
    assert info.status == "CONVERGED"
    Ws = np.stack([info.H_iter[-1], W0, ph.outside_W0(), W0])
    kw = dict(iters=2, eps=1e-3, gain_bias=False)
    Hs, infos = photo.PhotoTemplateMulti(t, masks).refine(f, Ws, active=[True, True, True, False], **kw)
    print("independent stopping:", [(i.status, len(i.cost)) if i is not None else None for i in infos])
    for k in range(3):
        pm.assert_same_refinement((Hs[k], infos[k]), photo.refine_homography(t, masks[k], f, Ws[k], **kw), k)
    assert (infos[0].status, len(infos[0].cost)) == ("CONVERGED", 2)
    assert (infos[1].status, len(infos[1].cost)) == ("MAX_ITERS", 3)
    assert (infos[2].status, infos[2].best, len(infos[2].cost), int(infos[2].n_valid[0])) == ("TOO_FEW", -1, 1, 0)
    assert np.array_equal(Hs[2], ph.outside_W0())
    assert infos[3] is None and np.array_equal(Hs[3], W0)


def _photo_calls(fn):
    fn_result = None
    _lib.load()
    with pytest.MonkeyPatch.context() as patch:
        proxy = U.CountingLib(_lib.load())
        patch.setattr(_lib, "_lib", proxy)
        fn_result = fn()
        torch.cuda.synchronize()
    return [c for c in proxy.calls if c.startswith("woft_photo")], fn_result


def test_no_call_when_no_target_takes_part(scene):
    t, f, W0 = scene["t"], scene["f"], scene["W0"]
    masks = pm.mask_set(3)
    multi = photo.PhotoTemplateMulti(t, masks)
    Ws = pm.poses(W0, 3)
    calls, (Hs, infos) = _photo_calls(lambda: multi.refine(f, Ws, active=[False, False, True]))   # (the third: never launchable)
    assert calls == [] and np.array_equal(Hs, Ws) and infos[0] is None and infos[1] is None
    assert (infos[2].status, infos[2].best, len(infos[2].cost)) == ("TOO_FEW", -1, 0)
    calls, (Hs, infos) = _photo_calls(lambda: multi.refine(f, Ws, active=[False] * 3))
    assert calls == [] and infos == [None] * 3 and np.array_equal(Hs, Ws)
    empty = photo.PhotoTemplateMulti(t, [np.zeros_like(masks[0]), masks[2]])
    calls, (Hs, infos) = _photo_calls(lambda: empty.refine(f, Ws[:2]))
    assert calls == [] and [i.status for i in infos] == ["TOO_FEW"] * 2 and np.array_equal(Hs, Ws[:2])


def test_one_call_and_one_read_whatever_k(scene):
    t, f, W0 = scene["t"], scene["f"], scene["W0"]
    for K in (1, 32):
        multi = photo.PhotoTemplateMulti(t, pm.mask_set(K))
        Ws = pm.poses(W0, K)
        multi.refine(f, Ws)                                                   # (buffers allocated)
        reads = []
        real = photo._Result.read

        def counted(self):
            reads.append(1)
            return real(self)
        with pytest.MonkeyPatch.context() as patch:
            patch.setattr(photo._Result, "read", counted)
            calls, _ = _photo_calls(lambda: multi.refine(f, Ws))
        assert calls == ["woft_photo_refine_multi"] and len(reads) == 1, (K, calls, reads)


def test_two_calls_give_equal_bytes(scene):
    t, f, W0 = scene["t"], scene["f"], scene["W0"]
    K, iters = 32, 10
    multi = photo.PhotoTemplateMulti(t, pm.mask_set(K))
    Ws = pm.poses(W0, K)
    active = [int(multi._launchable(k, 10)) for k in range(K)]
    active[5] = 0
    n_need = [max(10, (n + 1) // 2) for n in multi.n_sets]
    blocks, evals = [], []
    for _ in range(2):
        res = torch.full((K * ops.PHOTO_REC * (iters + 2),), float("nan"), dtype=torch.float64, device="cuda")
        ops.photo_refine_multi(multi.template, multi.bits, None, dev(f), multi._call_boxes, 1, Ws, n_need, active, iters, True, 6.0, 1e-3,
                               res)
        blocks.append(res.cpu().numpy().reshape(K, -1))
        out = torch.full((K, ops.PHOTO_NACC), float("nan"), dtype=torch.float64, device="cuda")
        ops.photo_eval_multi(multi.template, multi.bits, None, dev(f), multi._call_boxes, 1, Ws, [1.0] * K, [0.0] * K, active, True, 6.0, out)
        evals.append(out.cpu().numpy())
    assert blocks[0].tobytes() == blocks[1].tobytes() and evals[0].tobytes() == evals[1].tobytes()
    for k in range(K):
        blk = blocks[0][k]
        if not active[k]:                                                     # {SKIPPED, -1, 0} and nothing else
            assert blk[:3].tolist() == [5.0, -1.0, 0.0] and np.all(np.isnan(blk[3:])) and np.all(np.isnan(evals[0][k]))
        else:
            n_eval = int(blk[2])
            assert 1 <= n_eval <= iters + 1 and np.all(np.isnan(blk[ops.PHOTO_REC * (1 + n_eval):]))   # (later records not written)


def test_against_the_float64_restatement(scene):
    """Every recorded W_k of a K = 3 call against photo_host.refine per mask, by the rule of
    test_photo_gpu.py::test_refinement_six_iterations: the float32 restatement's own distance is the yardstick, the cost within
    photo_host.cost_tolerance."""
    t, f, W0 = scene["t"], scene["f"], scene["W0"]
    masks = [pm.mask_set(1)[0], pm.mask_set(3)[1], pm.mask_set(32)[31]]
    Ws = np.stack([W0] * 3)
    kw = dict(iters=6, eps=0.0)
    Hs, infos = photo.PhotoTemplateMulti(t, masks).refine(f, Ws, **kw)
    for k, m in enumerate(masks):
        ref, yard = ph.refine(t, m, f, W0, **kw), ph.refine(t, m, f, W0, dtype=np.float32, **kw)
        info, box = infos[k], ph.problem(t, m).box
        assert ref.margin > 1e-9, k
        assert len(info.cost) == len(ref.cost) == len(yard.cost), (k, len(info.cost), len(ref.cost), len(yard.cost))
        assert np.array_equal(info.n_valid, ref.n_valid) and np.array_equal(yard.n_valid, ref.n_valid), k
        for it in range(len(ref.cost)):
            d = ph.corner_distance(box, info.H_iter[it], ref.H_iter[it])
            y = ph.corner_distance(box, yard.H_iter[it], ref.H_iter[it])
            ctol = ph.cost_tolerance(ref.evals[it], *f.shape[:2])
            print(f"target {k} iterate {it}: kernel {d:.2e} px, float32 yardstick {y:.2e} px; |cost difference| "
                  f"{abs(info.cost[it] - ref.cost[it]):.2e}, bound {ctol:.2e}")
            assert d <= y, (k, it, d, y)
            assert abs(info.cost[it] - ref.cost[it]) <= ctol, (k, it)
        assert info.best == ref.best and np.array_equal(Hs[k], info.H_iter[info.best])
