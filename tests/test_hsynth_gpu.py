"""The synthetic-homography pair generator on the device: woft_hsynth_render and woft_hsynth_labels against
the float64 restatement of tests/hsynth_host.py, the existing warp kernel's bytes, repeat calls, the public interface
(woft_amd.hsynth) and the README's training loop on one HSynth sample.

Shapes: a 24x40 base image, destinations of 1x1, 3x5 and 17x33 pixels (one thread, a partial group of four pixels, a partial last
workgroup and a width that is no multiple of a thread's four pixels; every byte path of the stores, since 3x5 = 15 and 17x33 = 561
pixels are no multiple of four and the public wrappers' 24x40 labels are), occluder textures of 1x1 and 9x13, 0 / 1 / 2 (overlapping)
/ 4 occluders.  Run with -s for the measured maxima."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hsynth_host as hh  # noqa: E402
import mh_dense_host  # noqa: E402
from woft_amd import synth  # noqa: E402

GAINS = {"plain": (None, None), "photo": ((1.17, 0.83, 1.02), (-11.5, 7.25, 19.0))}


def render_tol(gain, bias):
    """32 * 2^-24 * max(255, 255 * max|gain| + max|bias|): the rounding of the dozen-odd float operations per channel (4 tap
    products and 3 blends of two products and a sum each, the gain and the bias, 3 operations per occluder on values that stay
    below that bound), each within 2^-24 relative."""
    g = 1.0 if gain is None else float(np.max(np.abs(gain)))
    b = 0.0 if bias is None else float(np.max(np.abs(bias)))
    return 32 * 2.0 ** -24 * max(255.0, 255.0 * g + b)


@pytest.fixture(scope="module")
def base():
    img = hh.base_image()
    return img, torch.from_numpy(img).cuda()


def _dev(occ):
    return [(torch.from_numpy(t).cuda(), H) for t, H in occ]


def _render(base_t, H, occ, gain, bias, out_hw):
    from woft_amd.hsynth import render_pair
    out = render_pair(base_t, H, _dev(occ), gain=gain, bias=bias, out_hw=out_hw, want_f32=True, want_cover=True)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("photo", list(GAINS))
@pytest.mark.parametrize("out_hw", hh.DST_HWS)
def test_render_against_float64(base, out_hw, photo):
    img, base_t = base
    gain, bias = GAINS[photo]
    tol = render_tol(gain, bias)
    worst, worst_c = 0.0, 0.0
    for hname, H in hh.homographies(out_hw).items():
        for n, occ in hh.occluder_sets(out_hw).items():
            u8, f32, cover = _render(base_t, H, occ, gain, bias, out_hw)
            want, want_c = hh.render(img, H, occ, gain, bias, out_hw)
            assert u8.shape == out_hw + (3,) and f32.shape == out_hw + (3,) and cover.shape == out_hw
            e = float(np.max(np.abs(f32.cpu().numpy().astype(np.float64) - want)))
            ec = float(np.max(np.abs(cover.cpu().numpy().astype(np.float64) - want_c)))
            worst, worst_c = max(worst, e), max(worst_c, ec)
            assert e <= tol, (hname, n, e, tol)
            assert ec <= 1e-6, (hname, n, ec)
            # the bytes are the rounding of the kernel's own float output: no near-tie allowance
            assert torch.equal(u8, torch.clamp(torch.round(f32), 0, 255).to(torch.uint8)), (hname, n)
            if n == 2 and out_hw == hh.DST_HWS[-1]:      # the order shows: the other way round is a different picture
                swapped, _ = hh.render(img, H, occ[::-1], gain, bias, out_hw)
                assert np.max(np.abs(swapped - want)) > 1.0
    print(f"\n[hsynth] render {out_hw} {photo}: max |out_f32 - f64| {worst:.3e} (bound {tol:.3e}), cover {worst_c:.3e}")


@pytest.mark.parametrize("out_hw", hh.DST_HWS + (hh.BASE_HW,))
def test_render_has_the_warp_kernel_bytes(base, out_hw):
    """No occluder, no gain, no bias: the bytes of ops.warp_perspective_u8 for the same image and matrix, and a zero cover.  (That
    kernel writes a destination of its image's size: for another size it runs on a canvas that holds the image and the
    destination -- zeros beyond the image are what the zero border samples -- and its top-left corner is compared.)"""
    from woft_amd import ops
    from woft_amd.hsynth import render_pair
    img, base_t = base
    for hname, H in hh.homographies(out_hw).items():
        u8, _, cover = render_pair(base_t, H, out_hw=out_hw, want_cover=True)
        assert float(cover.abs().max()) == 0.0
        if out_hw == hh.BASE_HW:
            want = torch.empty_like(base_t)
            ops.warp_perspective_u8(base_t, H, out=want)
            torch.cuda.synchronize()
            assert torch.equal(u8, want), hname
        else:
            # a destination of another size: the full-frame kernel on a canvas that holds both, cropped
            ch, cw = max(out_hw[0], img.shape[0]), max(out_hw[1], img.shape[1])
            canvas = torch.zeros((ch, cw, 3), dtype=torch.uint8, device="cuda")
            canvas[:img.shape[0], :img.shape[1]] = base_t
            want = torch.empty_like(canvas)
            ops.warp_perspective_u8(canvas, H, out=want)
            torch.cuda.synchronize()
            assert torch.equal(u8, want[:out_hw[0], :out_hw[1]]), hname


def _labels(H, occ, out_hw, **kw):
    from woft_amd.hsynth import pair_labels
    out = pair_labels(hh.BASE_HW, H, _dev(occ), out_hw=out_hw, **kw)
    torch.cuda.synchronize()
    return out


def test_labels_against_float64():
    """flow within one float32 ulp of the float64 value; visible and valid EQUAL to the restatement's (test_hsynth_cpu.py asserts
    the margins of exactly these inputs); beyond the horizon (d <= 0) not visible and valid."""
    worst = 0.0
    n_cases = 0
    for name, H, occ, out_hw in hh.label_cases():
        flow, visible, valid = _labels(H, occ, out_hw)
        f64, vis64, ok64, (px, py, d, T, inside) = hh.labels(hh.BASE_HW, H, occ, out_hw=out_hw, detail=True)
        assert flow.shape == (2,) + hh.BASE_HW and flow.dtype == torch.float32
        assert visible.shape == hh.BASE_HW and visible.dtype == torch.float32
        assert valid.shape == hh.BASE_HW and valid.dtype == torch.bool
        got = flow.cpu().numpy()
        ulp = np.spacing(np.abs(f64).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - f64) / ulp
        worst = max(worst, float(err.max()))
        assert float(err.max()) <= 1.0, name
        assert np.array_equal(visible.cpu().numpy().astype(np.float64), vis64), name
        assert np.array_equal(valid.cpu().numpy(), ok64), name
        if name.startswith("horizon"):
            beyond = d <= 0
            assert beyond.any() and (~beyond).any()
            assert not visible.cpu().numpy()[beyond].any() and valid.cpu().numpy()[beyond].all()
        n_cases += 1
    print(f"\n[hsynth] labels: {n_cases} cases, max flow error {worst:.3f} float32 ulp")


def _safe(px, py, d, T, inside, out_hw, lo, hi):
    """Template pixels whose labels rounding on the device cannot flip: test_hsynth_cpu.test_label_margins' margins, per pixel."""
    h, w = out_hw
    with np.errstate(invalid="ignore"):
        far = (np.abs(d) >= 1e-3) & (np.minimum(np.abs(px), np.abs(px - (w - 1))) >= 1e-6) \
            & (np.minimum(np.abs(py), np.abs(py - (h - 1))) >= 1e-6)
        return far & (~inside | ((np.abs(T - lo) >= 1e-4) & (np.abs(T - hi) >= 1e-4)))


def test_label_thresholds():
    """lo and hi are the caller's: the labels at (0.1, 0.9) are the restatement's at every pixel with the margins, and the wider
    band makes more pixels invalid and none more visible."""
    out_hw = hh.DST_HWS[-1]
    H, occ = hh.homographies(out_hw)["random0"], hh.occluder_sets(out_hw)[4]
    _, vis, ok = _labels(H, occ, out_hw, lo=0.1, hi=0.9)
    _, vis64, ok64, (px, py, d, T, inside) = hh.labels(hh.BASE_HW, H, occ, out_hw=out_hw, lo=0.1, hi=0.9, detail=True)
    safe = _safe(px, py, d, T, inside, out_hw, 0.1, 0.9)
    assert safe.mean() > 0.99
    assert np.array_equal(vis.cpu().numpy().astype(np.float64)[safe], vis64[safe])
    assert np.array_equal(ok.cpu().numpy()[safe], ok64[safe])
    _, vis_d, ok_d = _labels(H, occ, out_hw)
    assert int(ok.sum()) < int(ok_d.sum()) and int(vis.sum()) <= int(vis_d.sum())


def test_labels_of_an_odd_template():
    """A 5x7 template, 35 pixels: no multiple of a thread's four, so every store takes the float / byte path (flow's second plane
    would not be 16-byte aligned).  flow within one float32 ulp; visible and valid equal at every pixel with the margins."""
    from woft_amd.hsynth import pair_labels
    src_hw, out_hw = (5, 7), hh.DST_HWS[-1]
    H = np.array([[3.1, 0.2, 4.37], [-0.15, 2.9, 1.61], [0.002, -0.001, 1.0]])
    occ = hh.occluder_sets(out_hw)[2]
    flow, vis, ok = pair_labels(src_hw, H, _dev(occ), out_hw=out_hw)
    torch.cuda.synchronize()
    f64, vis64, ok64, (px, py, d, T, inside) = hh.labels(src_hw, H, occ, out_hw=out_hw, detail=True)
    ulp = np.spacing(np.abs(f64).astype(np.float32)).astype(np.float64)
    assert float((np.abs(flow.cpu().numpy().astype(np.float64) - f64) / ulp).max()) <= 1.0
    safe = _safe(px, py, d, T, inside, out_hw, 0.25, 0.75)
    assert safe.sum() >= 30 and 0 < vis64[safe].sum() < safe.sum()
    assert np.array_equal(vis.cpu().numpy().astype(np.float64)[safe], vis64[safe])
    assert np.array_equal(ok.cpu().numpy()[safe], ok64[safe])


def test_repeat_calls_and_optional_outputs(base):
    from woft_amd import ops
    img, base_t = base
    out_hw = hh.DST_HWS[-1]
    H, occ = hh.homographies(out_hw)["random1"], _dev(hh.occluder_sets(out_hw)[4])
    gain, bias = GAINS["photo"]

    def run(want_f32, want_cover, fill):
        u8 = torch.full(out_hw + (3,), fill, dtype=torch.uint8, device="cuda")
        f32 = torch.full(out_hw + (3,), float(fill), device="cuda") if want_f32 else None
        cover = torch.full(out_hw, float(fill), device="cuda") if want_cover else None
        ops.hsynth_render(base_t, H, occ, gain, bias, u8, f32, cover)
        torch.cuda.synchronize()
        return u8, f32, cover

    a, b = run(True, True, 0), run(True, True, 77)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    only_u8, only_f32, only_cover = run(False, False, 5), run(True, False, 9), run(False, True, 13)
    assert torch.equal(only_u8[0], a[0]) and torch.equal(only_f32[0], a[0]) and torch.equal(only_cover[0], a[0])
    assert torch.equal(only_f32[1], a[1]) and torch.equal(only_cover[2], a[2])
    la, lb = _labels(H, hh.occluder_sets(out_hw)[4], out_hw), _labels(H, hh.occluder_sets(out_hw)[4], out_hw)
    assert all(torch.equal(x, y) for x, y in zip(la, lb))


def test_unaligned_outputs_have_the_aligned_bytes(base):
    """Outputs that start one element into a buffer take the byte / float store path: the same values."""
    from woft_amd import ops
    img, base_t = base
    out_hw = (16, 24)                                       # a multiple of four pixels: the aligned call stores dwords
    H, occ = hh.homographies(out_hw)["random0"], _dev(hh.occluder_sets(out_hw)[2])
    n = out_hw[0] * out_hw[1]
    u8, f32, cover = (torch.empty(out_hw + (3,), dtype=torch.uint8, device="cuda"), torch.empty(out_hw + (3,), device="cuda"),
                      torch.empty(out_hw, device="cuda"))
    ops.hsynth_render(base_t, H, occ, None, None, u8, f32, cover)
    u8b, f32b, coverb = (torch.full((3 * n + 1,), 7, dtype=torch.uint8, device="cuda"), torch.full((3 * n + 1,), 7.0, device="cuda"),
                         torch.full((n + 1,), 7.0, device="cuda"))
    ops.hsynth_render(base_t, H, occ, None, None, u8b[1:].view(out_hw + (3,)), f32b[1:].view(out_hw + (3,)),
                      coverb[1:].view(out_hw))
    torch.cuda.synchronize()
    assert torch.equal(u8b[1:], u8.reshape(-1)) and torch.equal(f32b[1:], f32.reshape(-1)) and torch.equal(coverb[1:], cover.reshape(-1))
    assert int(u8b[0]) == 7 and float(f32b[0]) == 7.0 and float(coverb[0]) == 7.0


# ---- through the public interface ----------------------------------------------------------------------------------------------
SIZE = (128, 160)


@pytest.fixture(scope="module")
def images():
    return [synth.make_template(SIZE[0], SIZE[1], seq_id=k) for k in range(2)]


def _bytes(s):
    torch.cuda.synchronize()
    return [s.src.cpu().numpy().tobytes(), s.dst.cpu().numpy().tobytes(), s.H_gt.tobytes(), s.flow_gt.cpu().numpy().tobytes(),
            s.visible.cpu().numpy().tobytes(), s.valid.cpu().numpy().tobytes()]


def test_dataset(images):
    import woft_amd
    from woft_amd.hsynth import HSynth, HSynthSample, render_pair
    assert woft_amd.HSynth is HSynth and woft_amd.render_pair is render_pair
    ds = HSynth(images, seed=3, n_occluders=(1, 2))
    assert len(ds) == 2
    s0, s0b, s1 = ds[0], ds[0], ds[1]
    assert isinstance(s0, HSynthSample) and s0.H_gt.dtype == np.float64 and s0.H_gt.shape == (3, 3)
    assert s0.src.is_cuda and s0.dst.is_cuda and s0.dst.dtype == torch.uint8 and s0.dst.shape == SIZE + (3,)
    assert s0.flow_gt.shape == (2,) + SIZE and s0.visible.shape == SIZE and s0.valid.dtype == torch.bool
    assert _bytes(s0) == _bytes(s0b)
    assert all(a != b for a, b in zip(_bytes(s0)[1:], _bytes(s1)[1:]))
    assert _bytes(ds.sample(0, 1))[1] != _bytes(s0)[1] and _bytes(ds.sample(0, 0)) == _bytes(s0)
    assert _bytes(HSynth(images, seed=4, n_occluders=(1, 2))[0])[1] != _bytes(s0)[1]
    # the labels say something: occluded pixels, soft edges, pixels that leave the frame, and mostly visible ones
    vis, ok = s0.visible.cpu().numpy(), s0.valid.cpu().numpy()
    assert 0.3 < vis.mean() < 1.0 and (~ok).any() and ((vis == 0) & ok).any()
    # a numpy image and its device copy
    H = s0.H_gt
    a = render_pair(images[0], H, gain=1.1, bias=-3)
    b = render_pair(torch.from_numpy(images[0]).cuda(), H, gain=1.1, bias=-3)
    assert torch.equal(a, b)


def test_wrong_inputs(images):
    from woft_amd.hsynth import pair_labels, render_pair
    dev = torch.from_numpy(images[0]).cuda()
    tex = torch.zeros((4, 4, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError, match="base"):
        render_pair(dev.float(), np.eye(3))
    with pytest.raises(ValueError, match="base"):
        render_pair(dev.cpu(), np.eye(3))
    with pytest.raises(ValueError, match="base"):
        render_pair(dev[..., :2], np.eye(3))
    with pytest.raises(ValueError, match="H_gt"):
        render_pair(dev, np.eye(4))
    with pytest.raises(ValueError, match="gain"):
        render_pair(dev, np.eye(3), gain=(1.0, 2.0))
    with pytest.raises(ValueError, match=r"occluders\[0\] texture"):
        render_pair(dev, np.eye(3), [(tex[..., :3], np.eye(3))])
    with pytest.raises(ValueError, match="occluders"):
        render_pair(dev, np.eye(3), [(tex, np.eye(3))] * 5)
    with pytest.raises(ValueError, match="lo, hi"):
        pair_labels(SIZE, np.eye(3), lo=0.8, hi=0.2)
    with pytest.raises(ValueError, match="src_hw"):
        pair_labels((0, 4), np.eye(3))


# ---- the loop ------------------------------------------------------------------------------------------------------------------
STRUCTURE = [(32, 3)]
LR, STEPS = 1e-3, 40


def _provider(seed):
    from test_mh_dense_gpu import _config
    from woft_amd.flow_provider import RAFTWrapper
    sd = synth.make_state_dict(seed=seed, mask_head_structure=STRUCTURE)
    return RAFTWrapper(_config(sd, structure=STRUCTURE))


def test_sample_goes_through_compute_flow_and_the_loop_learns(images):
    """One fixed HSynth sample with two occluders through the README's loop (visibility_map, BCE with logits on the valid pixels,
    Adam, 40 steps): every gradient finite, the last loss below the first, two runs from the same start give the same bytes.
    The learning rate was chosen with the float32 torch restatement of the head (tests/mh_dense_host.py) on the same frozen
    inputs, whose loss has to fall by at least a third here; the kernels then only have to fall at all."""
    import torch.nn.functional as F
    from test_mh_dense_gpu import _frozen_inputs
    from woft_amd.hsynth import HSynth
    ds = HSynth(images, seed=3, n_occluders=(2, 2))
    s = ds[0]
    before = _bytes(s)
    p = _provider(7)
    flow = torch.as_tensor(p.compute_flow(s.src, s.dst, mode="flow")[0]).cpu()
    flow_np = torch.as_tensor(p.compute_flow(s.src.cpu().numpy(), s.dst.cpu().numpy(), mode="flow")[0]).cpu()
    assert flow.shape == (2,) + SIZE and torch.equal(flow, flow_np) and _bytes(s) == before
    params = list(p.mask_head_parameters().values())
    start = [q.detach().clone() for q in params]
    valid, target = s.valid, s.visible
    assert 0 < int(valid.sum()) and 0.0 < float(target[valid].mean()) < 1.0

    def run():
        with torch.no_grad():
            for q, q0 in zip(params, start):
                q.copy_(q0)
                q.grad = None
        opt = torch.optim.Adam(params, lr=LR)
        losses = []
        for _ in range(STEPS):
            p.compute_flow(s.src, s.dst, mode="flow")
            logits = p.visibility_map()
            loss = F.binary_cross_entropy_with_logits(logits[valid], target[valid])
            opt.zero_grad()
            loss.backward()
            assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in params)
            opt.step()
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        return losses, [q.detach().cpu().numpy().tobytes() for q in params]

    losses_a, final_a = run()
    losses_b, final_b = run()
    # the float32 torch restatement on the same frozen inputs and labels, on the host
    p.compute_flow(s.src, s.dst, mode="flow")
    x, mask, hf, wf, crop = _frozen_inputs(p)
    host_params = [q0.cpu().clone().requires_grad_(True) for q0 in start]
    opt = torch.optim.Adam(host_params, lr=LR)
    valid_h, target_h = valid.cpu(), target.cpu()
    host_losses = []
    for _ in range(STEPS):
        logits = mh_dense_host.visibility_map(x, host_params, mask, hf, wf, crop, SIZE[0], SIZE[1])
        loss = F.binary_cross_entropy_with_logits(logits[valid_h], target_h[valid_h])
        opt.zero_grad()
        loss.backward()
        opt.step()
        host_losses.append(float(loss.detach()))
    print(f"\n[hsynth] loop lr {LR}: kernels {losses_a[0]:.4f} -> {losses_a[-1]:.4f}, "
          f"float32 torch restatement {host_losses[0]:.4f} -> {host_losses[-1]:.4f}")
    assert host_losses[-1] <= (2.0 / 3.0) * host_losses[0]
    assert all(np.isfinite(losses_a)) and losses_a[-1] < losses_a[0]
    assert final_a == final_b and losses_a == losses_b
    with torch.no_grad():
        for q, q0 in zip(params, start):
            q.copy_(q0)


@pytest.mark.parametrize("head", ["mask", "weight"])
def test_train_heads_tool(head, tmp_path, capsys):
    """tools/train_heads.py, in this process: three steps on two 128x160 textures print three finite losses, and the saved file
    holds the head's parameters under the reference's state-dict names."""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    try:
        import train_heads
    finally:
        sys.path.pop(0)
    out = tmp_path / "head.pt"
    train_heads.main(["--head", head, "--size", "128", "160", "--textures", "2", "--steps", "3", "--iters", "4", "--lr", "1e-4",
                      "--out", str(out)])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step")]
    assert len(lines) == 3 and all("loss" in ln and np.isfinite(float(ln.split()[-1])) for ln in lines), lines
    saved = torch.load(out)
    prefix = "mask_head.net." if head == "mask" else "weight_head.net."
    assert saved and all(k.startswith(prefix) and v.dtype == torch.float32 for k, v in saved.items())
