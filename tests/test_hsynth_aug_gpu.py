"""The background and the photometric augmentation of the pair generator on the device:
woft_hsynth_render_bg and woft_hsynth_augment against the float64 restatement of tests/hsynth_aug_host.py, the old render's bytes,
identity parameters, in-place and repeat calls, the noise's independence of the other stages, the blur's replicate border, and
HSynth with the new keywords off (the parent's bytes) and on.

Shapes: the 24x40 base image, destinations of 1x1, 3x5 and 17x33 pixels (one thread, a partial group of four, a partial
workgroup; 3x5 is smaller than a radius-7 halo, so every tap clamps) and 40x72: the blur's tile is 32 x 32 pixels, so 72 columns are
two tiles and a partial one and 40 rows one tile and a partial one (a larger tile would need a larger frame; this one does not).
17x33 has one column in a second tile and rows whose first pixel is not 4-aligned in the flattened frame (the byte / float store
path), 40x72 takes the dword path.  Backgrounds of 1x1 and 11x7, radii 0, 1 and 7, 0 and 2 occluders.  Run with -s for the maxima."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hsynth_aug_host as ah  # noqa: E402
import hsynth_host as hh  # noqa: E402
from woft_amd import synth  # noqa: E402

GAINS = {"plain": (None, None), "photo": ((1.17, 0.83, 1.02), (-11.5, 7.25, 19.0))}
COLOUR = (0.6, 0.9, 1.3)            # saturation, hue, contrast of the "with colour" cases
NOISE = 6.0


def render_bg_tol(gain, bias):
    """(32 + 3) * 2^-24 * max(255, 255 * max|gain| + max|bias|): test_hsynth_gpu.render_tol's count of float operations per channel
    and its magnitude (v + (1 - P) g is a convex combination of values up to 255) plus the subtraction, the multiply and the add of
    the composite."""
    g = 1.0 if gain is None else float(np.max(np.abs(gain)))
    b = 0.0 if bias is None else float(np.max(np.abs(bias)))
    return (32 + 3) * 2.0 ** -24 * max(255.0, 255.0 * g + b)


@pytest.fixture(scope="module")
def base():
    img = hh.base_image()
    return img, torch.from_numpy(img).cuda()


def _dev(occ):
    return [(torch.from_numpy(t).cuda(), H) for t, H in occ]


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _round(f32):
    return torch.clamp(torch.round(f32), 0, 255).to(torch.uint8)


# ---- the background ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("photo", list(GAINS))
@pytest.mark.parametrize("out_hw", ah.AUG_HWS)
def test_background_against_float64(base, out_hw, photo):
    from woft_amd.hsynth import render_pair
    img, base_t = base
    gain, bias = GAINS[photo]
    tol = render_bg_tol(gain, bias)
    worst, worst_p, shown = 0.0, 0.0, False
    for bname, bg in ah.backgrounds().items():
        H_bg = ah.background_H(bg, out_hw)
        for hname, H in hh.homographies(out_hw).items():
            for n in (0, 2):
                occ = hh.occluder_sets(out_hw)[n]
                u8, f32, cover, plane = render_pair(base_t, H, _dev(occ), gain=gain, bias=bias, out_hw=out_hw, want_f32=True,
                                                    want_cover=True, background=bg, background_H=H_bg, want_plane=True)
                torch.cuda.synchronize()
                want, want_c, want_p = ah.render_bg(img, H, bg, H_bg, occ, gain, bias, out_hw)
                assert u8.shape == out_hw + (3,) and f32.shape == out_hw + (3,) and cover.shape == out_hw == plane.shape
                e = float(np.max(np.abs(_np(f32) - want)))
                ep = max(float(np.max(np.abs(_np(plane) - want_p))), float(np.max(np.abs(_np(cover) - want_c))))
                worst, worst_p = max(worst, e), max(worst_p, ep)
                assert e <= tol, (bname, hname, n, e, tol)
                assert ep <= 1e-6, (bname, hname, n, ep)
                assert torch.equal(u8, _round(f32)), (bname, hname, n)
                shown |= bool((want_p < 0.5).any() and (want_p > 0.5).any())
    assert shown or out_hw == (1, 1)                     # the background shows somewhere and the plane somewhere
    print(f"\n[hsynth-aug] background {out_hw} {photo}: max |out_f32 - f64| {worst:.3e} (bound {tol:.3e}), plane / cover {worst_p:.3e}")


@pytest.mark.parametrize("out_hw", ah.AUG_HWS)
def test_background_hidden_and_alone(base, out_hw):
    """A plane that covers the whole frame: the bytes (and floats) of woft_hsynth_render on the same arguments, plane = 1.  A
    plane wholly outside: gain * g + bias of the background within the bound, plane = 0."""
    from woft_amd.hsynth import render_pair
    img, base_t = base
    gain, bias = GAINS["photo"]
    bg = ah.backgrounds()["11x7"]
    H_bg = ah.background_H(bg, out_hw)
    occ = hh.occluder_sets(out_hw)[2]
    # the base image's interior stretched well beyond the frame
    hs, ws = hh.BASE_HW
    cover_all = np.array([[4.0 * max(out_hw[1], 2) / ws, 0.0, -1.5 * max(out_hw[1], 2)],
                          [0.0, 4.0 * max(out_hw[0], 2) / hs, -1.5 * max(out_hw[0], 2)], [0.0, 0.0, 1.0]])
    a = render_pair(base_t, cover_all, _dev(occ), gain=gain, bias=bias, out_hw=out_hw, want_f32=True, want_cover=True)
    b = render_pair(base_t, cover_all, _dev(occ), gain=gain, bias=bias, out_hw=out_hw, want_f32=True, want_cover=True,
                    background=bg, background_H=H_bg, want_plane=True)
    torch.cuda.synchronize()
    assert float(b[3].min()) == 1.0 and float(b[3].max()) == 1.0
    assert all(torch.equal(x, y) for x, y in zip(a, b[:3]))
    away = np.array([[1.0, 0.0, 1000.0], [0.0, 1.0, 1000.0], [0.0, 0.0, 1.0]])
    _, f32, _, plane = render_pair(base_t, away, gain=gain, bias=bias, out_hw=out_hw, want_f32=True, background=bg,
                                   background_H=H_bg, want_plane=True)
    torch.cuda.synchronize()
    g = ah.background_at(bg, H_bg, out_hw)
    assert float(plane.abs().max()) == 0.0
    assert float(np.max(np.abs(_np(f32) - (np.asarray(gain) * g + np.asarray(bias))))) <= render_bg_tol(gain, bias)


def test_background_optional_outputs_and_inputs(base):
    from woft_amd.hsynth import render_pair
    img, base_t = base
    out_hw = hh.DST_HWS[-1]
    bg = ah.backgrounds()["11x7"]
    H = hh.homographies(out_hw)["random1"]
    full = render_pair(base_t, H, out_hw=out_hw, want_f32=True, want_cover=True, background=bg, want_plane=True)
    only = render_pair(base_t, H, out_hw=out_hw, background=torch.from_numpy(bg).cuda(), background_H=np.eye(3))
    assert isinstance(only, torch.Tensor) and torch.equal(only, full[0])
    three = render_pair(base_t, H, out_hw=out_hw, want_cover=True, background=bg)
    assert len(three) == 3 and three[1] is None and torch.equal(three[2], full[2])
    with pytest.raises(ValueError, match="background"):
        render_pair(base_t, H, want_plane=True)
    with pytest.raises(ValueError, match="background"):
        render_pair(base_t, H, background=bg[..., :2])
    with pytest.raises(ValueError, match="background_H"):
        render_pair(base_t, H, background=bg, background_H=np.eye(4))


# ---- augment -------------------------------------------------------------------------------------------------------------------
def _augment(frame_t, radius, colour, noise_sigma, seed=5):
    from woft_amd.hsynth import augment
    s, hue, k = COLOUR if colour else (1.0, 0.0, 1.0)
    out = augment(frame_t, blur_sigma=ah.SIGMA_OF_RADIUS[radius], saturation=s, hue=hue, contrast=k, noise_sigma=noise_sigma,
                  seed=seed, want_f32=True)
    torch.cuda.synchronize()
    return out


def _host_params(radius, colour):
    from woft_amd.hsynth import blur_taps, colour_matrix
    taps = blur_taps(ah.SIGMA_OF_RADIUS[radius])
    assert (len(taps) - 1) // 2 == radius
    M, o = colour_matrix(*COLOUR)
    return (None if radius == 0 else taps), (np.concatenate([M.ravel(), o]).astype(np.float32) if colour else None)


@pytest.mark.parametrize("radius", ah.RADII)
@pytest.mark.parametrize("out_hw", ah.AUG_HWS)
def test_augment_against_float64(out_hw, radius):
    frame = ah.float_frame(out_hw)
    frame_t = torch.from_numpy(frame).cuda()
    for colour in (False, True):
        for noise_sigma in (0.0, NOISE):
            u8, f32 = _augment(frame_t, radius, colour, noise_sigma)
            taps, cm = _host_params(radius, colour)
            want, mag = ah.augment(frame, taps, cm, noise_sigma, seed=5, detail=True)
            tol = ah.augment_tol(radius, mag, noise_sigma)
            e = float(np.max(np.abs(_np(f32) - want)))
            print(f"\n[hsynth-aug] augment {out_hw} r={radius} colour={colour} noise={noise_sigma}: max |out_f32 - f64| {e:.3e} "
                  f"(bound {tol:.3e})", end="")
            assert e <= tol, (colour, noise_sigma, e, tol)
            assert torch.equal(u8, _round(f32)), (colour, noise_sigma)
    assert torch.equal(frame_t, torch.from_numpy(frame).cuda())          # the input is left as it was


@pytest.mark.parametrize("out_hw", ah.AUG_HWS)
def test_augment_identity_in_place_repeat_and_seed(out_hw):
    from woft_amd import ops
    from woft_amd.hsynth import augment
    frame = ah.float_frame(out_hw, seed=1)
    frame_t = torch.from_numpy(frame).cuda()
    # identity parameters: the rounding of the input, from a float32 and from a uint8 frame
    assert torch.equal(augment(frame_t), _round(frame_t))
    assert torch.equal(augment(_round(frame_t)), _round(frame_t))
    # radius 0 in place has the bytes of the out-of-place call
    _, cm = _host_params(0, True)
    u8a, f32a = torch.empty(out_hw + (3,), dtype=torch.uint8, device="cuda"), torch.empty_like(frame_t)
    ops.hsynth_augment(frame_t, None, cm, NOISE, 9, u8a, f32a)
    work, u8b = frame_t.clone(), torch.empty_like(u8a)
    ops.hsynth_augment(work, None, cm, NOISE, 9, u8b, work)
    torch.cuda.synchronize()
    assert torch.equal(u8a, u8b) and torch.equal(f32a, work)
    # with a blur in place is refused before any launch
    from woft_amd._lib import WoftHipError
    with pytest.raises(WoftHipError):
        ops.hsynth_augment(work, np.array([0.25, 0.5, 0.25], np.float32), None, 0.0, 0, u8b, work)
    for radius in ah.RADII:
        a, b = _augment(frame_t, radius, True, NOISE, seed=9), _augment(frame_t, radius, True, NOISE, seed=9)
        c = _augment(frame_t, radius, True, NOISE, seed=10)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert not torch.equal(a[1], c[1])
        # without the optional output: the same bytes
        s, hue, k = COLOUR
        only = augment(frame_t, blur_sigma=ah.SIGMA_OF_RADIUS[radius], saturation=s, hue=hue, contrast=k, noise_sigma=NOISE, seed=9)
        assert torch.equal(only, a[0])


def test_unaligned_outputs_have_the_aligned_bytes():
    """Outputs (and, without a blur, an input) that start one element into a buffer take the byte / float path: the same values."""
    from woft_amd import ops
    out_hw = ah.AUG_HWS[-1]
    n = out_hw[0] * out_hw[1]
    frame_t = torch.from_numpy(ah.float_frame(out_hw, seed=2)).cuda()
    shifted_in = torch.empty(3 * n + 1, device="cuda")
    shifted_in[1:] = frame_t.reshape(-1)
    _, cm = _host_params(0, True)
    for radius in (0, 7):
        taps, _ = _host_params(radius, True)
        u8, f32 = torch.empty(out_hw + (3,), dtype=torch.uint8, device="cuda"), torch.empty_like(frame_t)
        ops.hsynth_augment(frame_t, taps, cm, NOISE, 3, u8, f32)
        u8b, f32b = torch.full((3 * n + 1,), 7, dtype=torch.uint8, device="cuda"), torch.full((3 * n + 1,), 7.0, device="cuda")
        ops.hsynth_augment(shifted_in[1:].view(out_hw + (3,)), taps, cm, NOISE, 3, u8b[1:].view(out_hw + (3,)),
                           f32b[1:].view(out_hw + (3,)))
        torch.cuda.synchronize()
        assert torch.equal(u8b[1:], u8.reshape(-1)) and torch.equal(f32b[1:], f32.reshape(-1)), radius
        assert int(u8b[0]) == 7 and float(f32b[0]) == 7.0


@pytest.mark.parametrize("out_hw", ah.AUG_HWS)
def test_noise_is_independent_of_blur_and_colour(out_hw):
    """out_f32(noise) - out_f32(no noise) is sigma * z at every pixel and channel, whatever the blur and the colour map: within
    two float32 roundings of |u| (the add's own and the subtraction's here) plus the rounding of sigma * z."""
    frame = ah.float_frame(out_hw, seed=3)
    frame_t = torch.from_numpy(frame).cuda()
    z = ah.noise_z(5, *out_hw)
    for radius in ah.RADII:
        for colour in (False, True):
            _, with_noise = _augment(frame_t, radius, colour, NOISE)
            _, without = _augment(frame_t, radius, colour, 0.0)
            d = _np(with_noise) - _np(without)
            mag = np.maximum(np.abs(_np(with_noise)), np.abs(_np(without)))
            tol = 2 * 2.0 ** -24 * mag + 2 * 2.0 ** -24 * NOISE * ah.Z_MAX
            assert np.all(np.abs(d - NOISE * z) <= tol), (radius, colour, float(np.max(np.abs(d - NOISE * z) - tol)))


@pytest.mark.parametrize("radius", (1, 7))
def test_blur_edges(radius):
    """One bright pixel in a corner and one in the interior, both as the restatement has them.  The replicate border keeps the
    corner's mass inside the frame and counts it more than once: per axis the pixel weighs sum_{i <= 0} (|i| + 1) taps[i] instead
    of 1, so the sum over the frame exceeds the interior impulse's (the impulse's value) -- from radius 2 on; at radius 1 that
    weight is taps[0] + 2 taps[1] = 1 and the two sums agree.  A constant frame stays constant within 2 (2 r + 1) * 2^-24 * |v|."""
    h, w = 40, 72
    taps, _ = _host_params(radius, False)
    sums = {}
    for name, (y, x) in (("corner", (0, 0)), ("interior", (20, 36))):
        f = np.zeros((h, w, 3), np.float32)
        f[y, x] = 200.0
        _, f32 = _augment(torch.from_numpy(f).cuda(), radius, False, 0.0)
        want = ah.blur(f.astype(np.float64), taps)
        assert float(np.max(np.abs(_np(f32) - want))) <= ah.augment_tol(radius, 200.0, 0.0)
        sums[name] = float(_np(f32)[..., 0].sum())
        assert abs(sums[name] - float(want[..., 0].sum())) <= h * w * ah.augment_tol(radius, 200.0, 0.0)
    assert abs(sums["interior"] - 200.0) <= 1e-3
    assert sums["corner"] > sums["interior"] + 1.0 if radius > 1 else abs(sums["corner"] - sums["interior"]) <= 1e-3
    for hw in ((3, 5), (40, 72)):
        v = 173.3
        _, f32 = _augment(torch.full(hw + (3,), v, device="cuda"), radius, False, 0.0)
        assert float((f32 - np.float32(v)).abs().max()) <= 2 * (2 * radius + 1) * 2.0 ** -24 * v


def test_wrong_inputs():
    from woft_amd.hsynth import augment
    f = torch.zeros((8, 8, 3), device="cuda")
    with pytest.raises(TypeError, match="frame"):
        augment(f.double())
    with pytest.raises(TypeError, match="frame"):
        augment(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError, match="frame"):
        augment(f.cpu())
    with pytest.raises(ValueError, match="frame"):
        augment(f[..., :2])
    with pytest.raises(ValueError, match="noise_sigma"):
        augment(f, noise_sigma=-1.0)
    with pytest.raises(ValueError, match="seed"):
        augment(f, seed=1 << 32)
    with pytest.raises(ValueError, match="blur_sigma"):
        augment(f, blur_sigma=float("nan"))


# ---- HSynth --------------------------------------------------------------------------------------------------------------------
SIZE = (64, 96)


@pytest.fixture(scope="module")
def images():
    return [synth.make_template(SIZE[0], SIZE[1], seq_id=k) for k in range(2)]


def _bytes(s):
    torch.cuda.synchronize()
    return [s.src.cpu().numpy().tobytes(), s.dst.cpu().numpy().tobytes(), s.H_gt.tobytes(), s.flow_gt.cpu().numpy().tobytes(),
            s.visible.cpu().numpy().tobytes(), s.valid.cpu().numpy().tobytes()]


AUG = dict(blur_sigma=(0.5, 1.5), noise_sigma=(2.0, 5.0), saturation=(0.6, 1.4), hue=(-0.3, 0.3), contrast=(0.8, 1.2))


def _backgrounds():
    return [synth.make_template(40, 56, seq_id=11), ah.backgrounds()["11x7"]]


def test_dataset_defaults_are_the_parent_samples(images):
    """With every new keyword at its default a sample is render_pair + pair_labels on draw()'s four values: the parent's bytes."""
    from woft_amd.hsynth import HSynth, HSynthSample, pair_labels, render_pair
    ds = HSynth(images, seed=3, n_occluders=(1, 2))
    for i, e in ((0, 0), (1, 0), (0, 2)):
        drawn = ds.draw(i, e)
        assert len(drawn) == 4
        H_gt, occ, gain, bias = drawn[:4]
        occluders = [(ds.textures[t], H_occ) for t, H_occ in occ]
        dst = render_pair(ds.images[i], H_gt, occluders, gain=gain, bias=bias)
        flow, visible, valid = pair_labels(SIZE, H_gt, occluders, lo=ds.lo, hi=ds.hi)
        assert _bytes(ds.sample(i, e)) == _bytes(HSynthSample(ds.images[i], dst, H_gt, flow, visible, valid))


def test_dataset_augmented(images):
    from woft_amd.hsynth import HSynth, HSynthAugment
    plain = HSynth(images, seed=3, n_occluders=(1, 2))
    ds = HSynth(images, seed=3, n_occluders=(1, 2), backgrounds=_backgrounds(), **AUG)
    drawn = ds.draw(0, 0)
    assert len(drawn) == 5 and isinstance(drawn[4], HSynthAugment) and drawn[4].background in (0, 1)
    old = plain.draw(0, 0)
    assert np.array_equal(drawn[0], old[0]) and _same_occ(drawn[1], old[1]) and drawn[2:4] == old[2:4]
    for lo_hi, v in zip((AUG["blur_sigma"], AUG["saturation"], AUG["hue"], AUG["contrast"], AUG["noise_sigma"]), drawn[4][2:7]):
        assert lo_hi[0] <= v <= lo_hi[1]
    s, s_again, s_epoch, s_plain = ds.sample(0, 0), ds.sample(0, 0), ds.sample(0, 1), plain.sample(0, 0)
    assert s.dst.dtype == torch.uint8 and s.dst.shape == SIZE + (3,)
    assert _bytes(s) == _bytes(s_again) and _bytes(s)[1] != _bytes(s_epoch)[1]
    assert _bytes(s)[2:] == _bytes(s_plain)[2:]                       # H_gt, flow_gt, visible, valid
    assert _bytes(s)[1] != _bytes(s_plain)[1]
    assert _bytes(s)[0] == images[0].tobytes()
    # outside the plane and the occluders the plain pair is one flat colour (the bias); the augmented one has a scene there
    from woft_amd.hsynth import render_pair
    a = drawn[4]
    _, _, cover, plane = render_pair(images[0], drawn[0], [(ds.textures[t], Ho) for t, Ho in drawn[1]], want_cover=True,
                                     background=ds.backgrounds[a.background], background_H=a.background_H, want_plane=True)
    outside = (plane == 0) & (cover == 0)
    assert int(outside.sum()) > 20
    assert float(s_plain.dst[outside].float().std(0).max()) == 0.0 and float(s.dst[outside].float().std(0).min()) > 3.0
    # augment_src: src changes (its own noise seed), dst and the labels do not
    ds_src = HSynth(images, seed=3, n_occluders=(1, 2), backgrounds=_backgrounds(), augment_src=True, **AUG)
    t = ds_src.sample(0, 0)
    assert _bytes(t)[1:] == _bytes(s)[1:] and _bytes(t)[0] != _bytes(s)[0] and t.src.dtype == torch.uint8
    assert _bytes(ds_src.sample(0, 0))[0] == _bytes(t)[0]
    assert float((t.src.float() - s.src.float()).abs().mean()) < 40.0
    # one keyword alone switches the separate draws on and leaves the others at their identities
    noisy = HSynth(images, seed=3, n_occluders=(1, 2), noise_sigma=(3.0, 3.0))
    a = noisy.draw(0, 0)[4]
    assert a.background is None and a.background_H is None and (a.blur_sigma, a.saturation, a.hue, a.contrast) == (0, 1, 0, 1)
    n = noisy.sample(0, 0)
    assert _bytes(n)[2:] == _bytes(s_plain)[2:] and 0.5 < float((n.dst.float() - s_plain.dst.float()).abs().mean()) < 6.0


def _same_occ(a, b):
    return isinstance(a, list) and len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def test_dataset_refuses_wrong_keywords(images):
    from woft_amd.hsynth import HSynth
    with pytest.raises(ValueError, match=r"backgrounds\[0\]"):
        HSynth(images, backgrounds=[np.zeros((1, 5, 3), np.uint8)])
    with pytest.raises(TypeError, match=r"backgrounds\[0\]"):
        HSynth(images, backgrounds=[np.zeros((4, 5, 3), np.float32)])
    with pytest.raises(ValueError, match="noise_sigma"):
        HSynth(images, noise_sigma=(-1, 2))
    with pytest.raises(ValueError, match="blur_sigma"):
        HSynth(images, blur_sigma=(2, 1))


def test_mask_head_loop_on_an_augmented_sample(images):
    """The README's mask-head loop for 3 steps on one 64 x 96 augmented sample with a [(32, 3)] head: finite loss, finite and
    non-zero gradients."""
    import torch.nn.functional as F
    from test_hsynth_gpu import STRUCTURE, _provider
    from woft_amd.hsynth import HSynth
    assert STRUCTURE == [(32, 3)]
    ds = HSynth(images, seed=3, n_occluders=(2, 2), backgrounds=_backgrounds(), augment_src=True, **AUG)
    s = ds[0]
    p = _provider(7)
    params = list(p.mask_head_parameters().values())
    start = [q.detach().clone() for q in params]
    opt = torch.optim.Adam(params, lr=1e-3)
    assert 0 < int(s.valid.sum())
    for _ in range(3):
        p.compute_flow(s.src, s.dst, mode="flow")
        logits = p.visibility_map()
        loss = F.binary_cross_entropy_with_logits(logits[s.valid], s.visible[s.valid])
        opt.zero_grad()
        loss.backward()
        assert bool(torch.isfinite(loss))
        assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0 for q in params)
        opt.step()
    with torch.no_grad():
        for q, q0 in zip(params, start):
            q.copy_(q0)
            q.grad = None


def test_train_heads_tool_with_augmentation(tmp_path, capsys):
    """tools/train_heads.py with the new options, in this process: two steps print two finite losses."""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    try:
        import train_heads
    finally:
        sys.path.pop(0)
    bg = tmp_path / "bg.npy"
    np.save(bg, synth.make_template(40, 56, seq_id=11))
    out = tmp_path / "head.pt"
    train_heads.main(["--head", "mask", "--size", "64", "96", "--textures", "2", "--steps", "2", "--iters", "2", "--lr", "1e-4",
                      "--out", str(out), "--backgrounds", str(bg), "--blur", "0.5", "1.5", "--noise", "1", "4", "--saturation", "0.7",
                      "1.3", "--hue", "-0.2", "0.2", "--contrast", "0.9", "1.1", "--augment-src"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step")]
    assert len(lines) == 2 and all("loss" in ln and np.isfinite(float(ln.split()[-1])) for ln in lines), lines
    assert out.exists()
