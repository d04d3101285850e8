"""The photometric refinement on the device (csrc/photo.hip) against the float64 restatement of
tests/photo_host.py: single evaluations entry by entry against a derived rounding bound, the smallest shapes, whole refinements
iterate by iterate against the float32 restatement's own distance from the float64 one, the status cases, repeat calls and the
device generator end to end.  tests/test_photo_cpu.py asserts what these comparisons lean on.  Run with -s for the maxima."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import photo_host as ph  # noqa: E402
from woft_amd import ops, photo  # noqa: E402


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def eval_device(template, mask, weights, frame, box, stride, W, gain, bias_s, gain_bias, huber_k):
    out = torch.full((ops.PHOTO_NACC,), float("nan"), dtype=torch.float64, device="cuda")
    ops.photo_eval(dev(template), dev((mask > 0).astype(np.uint8)), dev(weights), dev(frame), box, stride, W, gain, bias_s, gain_bias,
                   huber_k, out)
    return out.cpu().numpy()


def check_eval(name, template, mask, frame, W, gain=1.05, bias_s=-12.0, gain_bias=True, huber_k=None, stride=1, weights=None):
    """One evaluation on the device against the restatement: n equal, every entry of G, r and the cost sums within the bound.
    -> the largest ratio error / bound."""
    P = ph.problem(template, mask, stride, weights)
    ev = ph.evaluate(P, ph.intensity(frame), ph.to_state(P, W), gain, bias_s, gain_bias, huber_k)
    assert ev.margin > 1e-9, name
    nu = 10 if gain_bias else 8
    acc = eval_device(template, mask, weights, frame, P.box, stride, W, gain, bias_s, gain_bias, huber_k)
    tri = nu * (nu + 1) // 2
    G, r, _, n = photo.unpack_sums(acc, nu)
    cs, ws = acc[tri + nu], acc[tri + nu + 1]
    tol = ph.eval_tolerances(ev, *frame.shape[:2])
    assert n == ev.n, (name, n, ev.n)
    worst = 0.0
    for what, got, ref, bound in (("G", G, ev.G, tol.G), ("r", r, ev.r, tol.r), ("cs", cs, ev.cs, tol.cs), ("ws", ws, ev.ws, tol.ws)):
        err, bound = np.abs(np.asarray(got) - np.asarray(ref)), np.asarray(bound)
        ratio = float(np.max(err / np.where(bound > 0, bound, 1.0))) if ev.n else 0.0
        worst = max(worst, ratio)
        assert np.all(err <= bound), (name, what, float(err.max()), ratio)
    return worst


@pytest.fixture(scope="module")
def base():
    t, m, f, H_gt, W0 = ph.base_case(ph.SEEDS[0])
    rs = np.random.RandomState(5)
    f32 = {"t": (t.astype(np.float32) * np.float32(0.97) + np.float32(1.3)),
           "f": (f.astype(np.float32) + rs.uniform(-0.5, 0.5, f.shape).astype(np.float32)),
           "w": rs.uniform(0.0, 2.0, m.shape).astype(np.float32)}
    f32["w"][rs.uniform(size=m.shape) < 0.1] = 0.0
    return t, m, f, H_gt, W0, f32


def test_single_evaluation_every_combination(base):
    t, m, f, _, W0, f32 = base
    worst = 0.0
    for tf, ff, wt, hk, stride, gb in itertools.product((False, True), (False, True), (False, True), (None, 6.0), (1, 2), (True, False)):
        name = f"template {'f32' if tf else 'u8'} frame {'f32' if ff else 'u8'} weights {wt} huber {hk} stride {stride} gain_bias {gb}"
        worst = max(worst, check_eval(name, f32["t"] if tf else t, m, f32["f"] if ff else f, W0, gain_bias=gb, huber_k=hk,
                                      stride=stride, weights=f32["w"] if wt else None))
    print(f"single evaluation, 64 combinations: largest error / bound {worst:.3f}")


def small_cases():
    rs = np.random.RandomState(21)
    img = lambda h, w: rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    shift = lambda dx, dy: np.array([[1.01, 0.02, dx], [-0.015, 0.99, dy], [1e-4, -2e-4, 1.0]])
    m = np.zeros((5, 7), np.uint8)
    m[1:4, 1:6] = 255
    yield "5x7, 15 interior pixels", img(5, 7), m, img(9, 11), shift(2.2, 1.7), 1
    yield "5x7, mask to the border", img(5, 7), np.full((5, 7), 255, np.uint8), img(9, 11), shift(2.2, 1.7), 1
    m = np.zeros((5, 40), np.uint8)
    m[2, 3:33] = 255
    yield "one-row mask", img(5, 40), m, img(9, 44), shift(1.3, 2.4), 1
    m = np.zeros((6, 1500), np.uint8)
    m[1:5, 1:1301] = 255                                             # (5200 candidates: chunks of 2048, 2048 and 1104)
    yield "strip over three workgroups", img(6, 1500), m, img(12, 1506), shift(2.6, 3.1), 1
    m = np.zeros((9, 1500), np.uint8)
    m[1:8, 1:1400] = 255
    yield "strip, stride 2 on odd extents", img(9, 1500), m, img(14, 1506), shift(2.6, 3.1), 2


def test_smallest_shapes():
    for name, t, m, f, W, stride in small_cases():
        P = ph.problem(t, m, stride)
        pt = photo.PhotoTemplate(t, m, stride=stride)
        assert pt.n_set == P.n_set and pt.box == P.box, name
        r = check_eval(name, t, m, f, W, stride=stride)
        print(f"{name}: n_set {P.n_set}, largest error / bound {r:.3f}")
    assert photo.PhotoTemplate(np.zeros((5, 7, 3), np.uint8), np.full((5, 7), 255, np.uint8)).n_set == 15


def test_too_few_without_a_launch():
    rs = np.random.RandomState(3)
    t, f = rs.randint(0, 256, (5, 7, 3)).astype(np.uint8), rs.randint(0, 256, (9, 11, 3)).astype(np.uint8)
    m = np.zeros((5, 7), np.uint8)
    m[1:4, 1:4] = 255
    W = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 2.0], [0.0, 0.0, 1.0]])
    H, info = photo.refine_homography(t, m, f, W)
    assert (info.status, info.best, len(info.cost), info.n_set) == ("TOO_FEW", -1, 0, 9) and np.array_equal(H, W)
    H, info = photo.refine_homography(t, m, f, W, gain_bias=False)                # (8 unknowns: nine pixels are launched)
    assert len(info.cost) >= 1
    H, info = photo.refine_homography(t, np.zeros((5, 7), np.uint8), f, W)
    assert (info.status, info.best, len(info.cost)) == ("TOO_FEW", -1, 0)


def compare_run(name, got, ref, yard, hw):
    """Iterate by iterate: W_k within the float32 restatement's own distance from the float64 one (no factor: the kernel is fp64),
    n_k equal, cost_k within the evaluation bound; best = the first minimum of the kernel's own costs, H that iterate's."""
    H, info = got
    assert len(info.cost) == len(ref.cost) == len(yard.cost), (name, len(info.cost), len(ref.cost))
    assert np.array_equal(info.n_valid, ref.n_valid) and np.array_equal(yard.n_valid, ref.n_valid), name
    worst = 0.0
    for k in range(len(ref.cost)):
        d = ph.corner_distance(ph.BOX, info.H_iter[k], ref.H_iter[k])
        y = ph.corner_distance(ph.BOX, yard.H_iter[k], ref.H_iter[k])
        ctol = ph.cost_tolerance(ref.evals[k], *hw)
        print(f"{name} iterate {k}: kernel {d:.2e} px, float32 yardstick {y:.2e} px; cost {info.cost[k]:.6f}, "
              f"|difference| {abs(info.cost[k] - ref.cost[k]):.2e}, bound {ctol:.2e}")
        assert d <= y, (name, k, d, y)
        assert abs(info.cost[k] - ref.cost[k]) <= ctol, (name, k)
        worst = max(worst, d)
    assert info.best == int(np.argmin(info.cost)) == ref.best, name
    assert np.array_equal(H, info.H_iter[info.best]) and info.rms_after <= info.rms_before, name
    assert info.rms_before == info.cost[0] and info.rms_after == info.cost[info.best]
    # (gain, bias and step: looser than the pose on purpose -- fp64 solves of one system, far inside the float32 yardstick's 1e-5)
    assert np.allclose(info.gain, ref.gain, rtol=0, atol=1e-7) and np.allclose(info.bias, ref.bias, rtol=0, atol=1e-5), name
    assert np.allclose(info.step[:-1], ref.step[:-1], rtol=0, atol=1e-7) and np.isnan(info.step[-1]), name
    return worst


@pytest.mark.parametrize("seed", ph.SEEDS)
@pytest.mark.parametrize("config", sorted(ph.CONFIGS))
def test_refinement_six_iterations(seed, config):
    t, m, f, H_gt, W0 = ph.base_case(seed)
    kw = dict(iters=6, eps=0.0, **ph.CONFIGS[config])
    ref, yard = ph.refine(t, m, f, W0, **kw), ph.refine(t, m, f, W0, dtype=np.float32, **kw)
    worst = compare_run(f"seed {seed} {config}", photo.refine_homography(t, m, f, W0, **kw), ref, yard, f.shape[:2])
    print(f"seed {seed} {config}: largest kernel distance {worst:.2e} px")


def test_refinement_without_gain_bias_and_with_stride(base):
    t, m, f, _, W0, _ = base
    for name, kw in (("no gain / bias", dict(gain_bias=False)), ("stride 2", dict(stride=2))):
        kw = dict(iters=6, eps=0.0, **kw)
        ref, yard = ph.refine(t, m, f, W0, **kw), ph.refine(t, m, f, W0, dtype=np.float32, **kw)
        compare_run(name, photo.refine_homography(t, m, f, W0, **kw), ref, yard, f.shape[:2])


def test_early_stop_matches(base):
    """eps = 1e-3: the status and the number of evaluated iterates are the restatement's."""
    for seed in ph.SEEDS:
        t, m, f, _, W0 = ph.base_case(seed)
        for config, cfg in ph.CONFIGS.items():
            ref = ph.refine(t, m, f, W0, **cfg)
            H, info = photo.refine_homography(t, m, f, W0, **cfg)
            print(f"seed {seed} {config}: {info.status} after {len(info.cost)} iterates (restatement {ref.status}, {len(ref.cost)})")
            assert (info.status, len(info.cost), info.best) == (ref.status, len(ref.cost), ref.best)
            assert np.array_equal(info.n_valid, ref.n_valid)
            assert ph.corner_distance(ph.BOX, H, ref.H) < 1e-6


def test_status_cases(base):
    t, m, f, _, W0, _ = base
    H, info = photo.refine_homography(np.full_like(t, 77), m, f, W0)
    assert (info.status, info.best, len(info.cost)) == ("SINGULAR", 0, 1) and ph.corner_distance(ph.BOX, H, W0) < 1e-9
    one = np.zeros_like(m)
    one[30, 40] = 255
    H, info = photo.refine_homography(t, one, f, W0)
    assert (info.status, info.best, len(info.cost)) == ("TOO_FEW", -1, 0) and np.array_equal(H, W0)
    H, info = photo.refine_homography(t, m, f, ph.outside_W0())
    assert (info.status, info.best, len(info.cost), int(info.n_valid[0])) == ("TOO_FEW", -1, 1, 0)
    assert np.array_equal(H, ph.outside_W0())
    # part of the mask outside the frame: n_valid changes between iterates and stays above the threshold
    t, m, f, _, W0 = ph.partial_case()
    ref = ph.refine(t, m, f, W0)
    H, info = photo.refine_homography(t, m, f, W0)
    assert (info.status, info.best, len(info.cost)) == (ref.status, ref.best, len(ref.cost))
    assert np.array_equal(info.n_valid, ref.n_valid) and len(set(info.n_valid.tolist())) > 1
    # ... and below it at a later iterate
    t, m, f, _, W0, mv = ph.shrinking_case()
    ref = ph.refine(t, m, f, W0, min_valid=mv)
    H, info = photo.refine_homography(t, m, f, W0, min_valid=mv)
    assert (info.status, info.best, len(info.cost)) == ("TOO_FEW", ref.best, len(ref.cost)) and len(info.cost) >= 2
    assert np.array_equal(info.n_valid, ref.n_valid) and np.array_equal(H, info.H_iter[info.best])


def test_two_calls_give_equal_bytes(base):
    t, m, f, _, W0, f32 = base
    P = ph.problem(t, m)
    a = eval_device(t, m, f32["w"], f, P.box, 1, W0, 1.05, -12.0, True, 6.0)
    b = eval_device(t, m, f32["w"], f, P.box, 1, W0, 1.05, -12.0, True, 6.0)
    assert a.tobytes() == b.tobytes()
    pt = photo.PhotoTemplate(t, m)
    blocks = []
    for _ in range(2):
        res = torch.full((ops.PHOTO_REC * 12,), float("nan"), dtype=torch.float64, device="cuda")
        ops.photo_refine(pt.template, pt.mask, None, dev(f), pt.box, 1, W0, 10, True, None, 1100, 1e-3, res)
        blocks.append(res.cpu().numpy())
    assert blocks[0].tobytes() == blocks[1].tobytes()
    n_eval = int(blocks[0][2])
    assert 2 <= n_eval <= 11 and np.all(np.isnan(blocks[0][ops.PHOTO_REC * (1 + n_eval):]))     # (later records are not written)


def test_device_generator_end_to_end():
    """render_pair of the base template under H_gt with gain and bias, refined from the perturbed pose: the corner error against
    H_gt is within the yardstick of the restatement's result on the same bytes.  Device tensors in, nothing uploaded twice."""
    from woft_amd import hsynth
    t, m, _, H_gt, W0 = ph.base_case(ph.SEEDS[1])
    frame = hsynth.render_pair(dev(t), H_gt, gain=ph.GAIN, bias=ph.BIAS, out_hw=ph.FRAME_HW)
    kw = dict(iters=6, eps=0.0)
    H, info = photo.PhotoTemplate(dev(t), dev(m)).refine(frame, W0, **kw)
    f = frame.cpu().numpy()
    ref, yard = ph.refine(t, m, f, W0, **kw), ph.refine(t, m, f, W0, dtype=np.float32, **kw)
    assert info.best == ref.best == yard.best
    e0, e_dev, e_ref = (ph.corner_distance(ph.BOX, X, H_gt) for X in (W0, H, ref.H))
    y = ph.corner_distance(ph.BOX, yard.H, ref.H)
    print(f"device generator: corner error {e0:.3f} -> {e_dev:.6f} px (restatement {e_ref:.6f}), |difference| {abs(e_dev - e_ref):.2e}, "
          f"yardstick {y:.2e}")
    assert abs(e_dev - e_ref) <= y and e_dev <= 0.25 * e0
