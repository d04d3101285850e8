"""woft_amd.hsynth.render_pair and pair_labels (csrc/hsynth.hip) at 1080p and 4K with 0 and 2 occluders, next to
what a user had before: the same arithmetic in torch ops on the device (fp64 coordinates, float32 taps gathered by index, the same
premultiplied compositing), and the float64 numpy restatement of tests/hsynth_host.py on the host plus the upload of its results.
One process, alternating rounds after one warm-up round, HIP events around each round's calls (the host side by the wall clock,
one call per round).  Next to each HIP figure its streaming floor, DERIVED from the bytes the call must move at the 6.29 TB/s this
project measured -- the kernels are bound by their fp64 divisions, not by bytes, and the floor says how far that is.  The lines go
to --out (profiles/hsynth_bench.txt).

--augment times what DESIGN.md section 24 added instead, in the same way (--out profiles/hsynth_augment_bench.txt): render_pair with
and without a background, and augment at radius 0, 2 and 7 with a colour map and noise next to the same arithmetic in torch ops on
the device (F.conv2d over a replicate-padded frame for the blur, a matmul for the colour map, the hash in int64 tensor ops)."""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch
import torch.nn.functional as F

import hsynth_host
from woft_amd import synth
from woft_amd.hsynth import augment, blur_taps, colour_matrix, make_occluder, pair_labels, random_homography, render_pair

STREAM_TBPS = 6.29


def _round(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def _taps(Hinv, xs, ys, h, w):
    """warp_pixel.h's coordinates in torch: fp64 source point, float32 fractions, flags and clamped flat indices of the 4 taps."""
    d = Hinv[2, 0] * xs + Hinv[2, 1] * ys + Hinv[2, 2]
    sx, sy = (Hinv[0, 0] * xs + Hinv[0, 1] * ys + Hinv[0, 2]) / d, (Hinv[1, 0] * xs + Hinv[1, 1] * ys + Hinv[1, 2]) / d
    fx0, fy0 = torch.floor(sx), torch.floor(sy)
    fx, fy = (sx - fx0).float(), (sy - fy0).float()
    x0, y0 = fx0.clamp(-4, w + 4).long(), fy0.clamp(-4, h + 4).long()
    taps = []
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            ok = ((xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)).float()
            taps.append((ok, yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)))
    return fx, fy, taps


def _blend(fx, fy, v):
    top, bot = v[0] * (1 - fx) + v[1] * fx, v[2] * (1 - fx) + v[3] * fx
    return top * (1 - fy) + bot * fy


def _sample(planes, Hinv, xs, ys):
    """planes (h, w, C) float32 at Hinv (xs, ys, 1), zero border -> (..., C)."""
    h, w, C = planes.shape
    fx, fy, taps = _taps(Hinv, xs, ys, h, w)
    flat = planes.reshape(-1, C)
    return _blend(fx[..., None], fy[..., None], [ok[..., None] * flat[i] for ok, i in taps])


def torch_render(base_f, Hinv, gain, bias, occ, grid):
    xs, ys = grid
    v = gain * _sample(base_f, Hinv, xs, ys) + bias
    keep = torch.ones_like(xs, dtype=torch.float32)
    for pre, Oinv in occ:
        s = _sample(pre, Oinv, xs, ys)
        A = s[..., 3]
        v = (1 - A)[..., None] * v + s[..., :3]
        keep = keep * (1 - A)
    return torch.clamp(torch.round(v), 0, 255).to(torch.uint8), v, 1 - keep


def torch_labels(Hf, occ, grid, h, w, lo=0.25, hi=0.75):
    xs, ys = grid
    d = Hf[2, 0] * xs + Hf[2, 1] * ys + Hf[2, 2]
    px, py = (Hf[0, 0] * xs + Hf[0, 1] * ys + Hf[0, 2]) / d, (Hf[1, 0] * xs + Hf[1, 1] * ys + Hf[1, 2]) / d
    flow = torch.stack([(px - xs).float(), (py - ys).float()])
    inside = (d > 0) & (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)
    keep = torch.ones_like(xs, dtype=torch.float32)
    for pre, Oinv in occ:
        keep = keep * (1 - _sample(pre[..., 3:], Oinv, px, py)[..., 0])
    T = 1 - keep
    seen = inside & (T <= lo)
    return flow, seen.float(), seen | ~inside | (T >= hi)


def _mix(v):
    m = 0xFFFFFFFF
    v = v ^ (v >> 16)
    v = (v * 0x7FEB352D) & m
    v = v ^ (v >> 15)
    v = (v * 0x846CA68B) & m
    return v ^ (v >> 16)


def torch_augment(frame, taps, M, o, sigma, seed):
    """woft_hsynth_augment's arithmetic in torch ops: frame (h, w, 3) float32 -> uint8.  (int64 products of two 32-bit values wrap
    in their upper bits only: the masked lower 32 are the uint32 product.)"""
    h, w = frame.shape[:2]
    t = frame
    if taps is not None:
        r = (taps.numel() - 1) // 2
        x = F.pad(frame.permute(2, 0, 1)[None], (r, r, r, r), mode="replicate")
        x = F.conv2d(x, taps.reshape(1, 1, 1, -1).expand(3, 1, 1, -1), groups=3)
        x = F.conv2d(x, taps.reshape(1, 1, -1, 1).expand(3, 1, -1, 1), groups=3)
        t = x[0].permute(1, 2, 0)
    u = t.reshape(-1, 3) @ M.t() + o
    idx = torch.arange(h * w * 3, device=frame.device, dtype=torch.int64) & 0xFFFFFFFF
    a = _mix(seed ^ _mix(idx))
    b = _mix((a + 0x9E3779B9) & 0xFFFFFFFF)
    S = (a & 0xFFFF) + (a >> 16) + (b & 0xFFFF) + (b >> 16)
    z = (S - 131070).float() * float(np.float32(np.sqrt(3.0) / 65536.0))
    u = u.reshape(-1) + sigma * z
    return torch.clamp(torch.round(u), 0, 255).to(torch.uint8).reshape(h, w, 3)


def bench_augment(args):
    med = lambda v: sorted(v)[len(v) // 2]
    span = lambda v: f"{med(v) * 1e3:9.1f} us ({min(v) * 1e3:.1f} - {max(v) * 1e3:.1f})"
    fl = lambda b: b / (STREAM_TBPS * 1e12) * 1e6
    lines = [f"woft_amd.hsynth render_pair with a background and augment on the device, augment next to torch ops on the device; "
             f"{args.rounds} alternating rounds of {args.reps} HIP / {args.torch_reps} torch calls each after one warm-up round, per "
             "call through the public wrappers (allocation of the outputs and the host's 3x3 inversions, taps and colour matrix "
             "included; back-to-back calls, a frame may stay in the Infinity Cache): median (min - max); floors are DERIVED from the "
             "byte counts at the measured 6.29 TB/s, not measured"]
    for H, W in zip(args.sizes[0::2], args.sizes[1::2]):
        base_d = torch.from_numpy(synth.make_template(H, W)).cuda()
        bg_d = torch.from_numpy(synth.make_template(H // 2 // 8 * 8, W // 2 // 8 * 8, seq_id=3)).cuda()
        rs = np.random.RandomState(1)
        H_gt = random_homography(rs, H, W, 0.2)
        H_bg = np.diag([2.2, 2.2, 1.0]) @ random_homography(rs, bg_d.shape[0], bg_d.shape[1], 0.1)
        H_bg[:2, 2] -= 0.1 * np.array([W, H])
        texs = [make_occluder(rs, 256, 320), make_occluder(rs, 192, 192)]
        place = lambda cx, cy, s: np.array([[s, 0, cx], [0, s, cy], [0, 0, 1.0]])
        occ_all = [(torch.from_numpy(texs[0]).cuda(), place(0.2 * W, 0.3 * H, H / 1080.0) @ random_homography(rs, 256, 320, 0.2)),
                   (torch.from_numpy(texs[1]).cuda(), place(0.5 * W, 0.4 * H, 1.5 * H / 1080.0) @ random_homography(rs, 192, 192, 0.2))]
        frame = render_pair(base_d, H_gt, occ_all, gain=1.1, bias=-5.0, want_f32=True, background=bg_d, background_H=H_bg)[1]
        sat, hue, con, sigma, seed = 0.7, 0.3, 1.2, 4.0, 12345
        M64, o64 = colour_matrix(sat, hue, con)
        M, o = torch.from_numpy(M64.astype(np.float32)).cuda(), torch.from_numpy(o64.astype(np.float32)).cuda()
        out = {}
        sides = []
        for n_occ in (0, 2):
            occ = occ_all[:n_occ]
            sides.append((f"render {n_occ} occ", lambda occ=occ: render_pair(base_d, H_gt, occ, gain=1.1, bias=-5.0), args.reps))
            sides.append((f"render_bg {n_occ} occ", lambda occ=occ: render_pair(base_d, H_gt, occ, gain=1.1, bias=-5.0, background=bg_d,
                                                                              background_H=H_bg), args.reps))
        blur_sigma = {0: 0.0, 2: 0.6, 7: 2.5}
        for r, bs in blur_sigma.items():
            taps = blur_taps(bs)
            assert (len(taps) - 1) // 2 == r
            taps_d = None if r == 0 else torch.from_numpy(taps).cuda()

            def hip(r=r, bs=bs):
                out[f"hip{r}"] = augment(frame, bs, sat, hue, con, sigma, seed)

            def tor(r=r, taps_d=taps_d):
                out[f"t{r}"] = torch_augment(frame, taps_d, M, o, sigma, seed)
            sides.append((f"augment r={r}", hip, args.reps))
            if not args.hip_only:
                sides.append((f"torch r={r}", tor, args.torch_reps))
        sides.append(("augment r=7 + out_f32", lambda: augment(frame, 2.5, sat, hue, con, sigma, seed, want_f32=True), args.reps))
        t = {k: [] for k, _, _ in sides}
        for rnd in range(args.rounds + 1):
            for label, fn, reps in sides:
                ms = _round(fn, reps)
                if rnd > 0:
                    t[label].append(ms)
        lines.append(f"{H} x {W} (background {bg_d.shape[0]} x {bg_d.shape[1]})")
        for n_occ in (0, 2):
            a, b = t[f"render {n_occ} occ"], t[f"render_bg {n_occ} occ"]
            bytes_r = 3 * H * W * 2 + bg_d.numel()                   # + the background region read once (here: at most all of it)
            lines.append(f"  render_pair, {n_occ} occluders  no background {span(a)} | with background {span(b)} = {med(b) / med(a):.2f} x | "
                         f"derived floor with background {fl(bytes_r):.1f} us ({bytes_r / 1e6:.1f} MB) = {med(b) * 1e3 / fl(bytes_r):.1f} x")
        for r in blur_sigma:
            bytes_a = 15 * H * W                                     # 12 B read + 3 B written per pixel
            line = f"  augment radius {r}, colour, noise  HIP {span(t[f'augment r={r}'])} | derived floor {fl(bytes_a):.1f} us " \
                   f"({bytes_a / 1e6:.1f} MB) = {med(t[f'augment r={r}']) * 1e3 / fl(bytes_a):.1f} x"
            if not args.hip_only:
                diff = int((out[f"hip{r}"].int() - out[f"t{r}"].int()).abs().max())
                line += f" | torch ops {span(t[f'torch r={r}'])} = {med(t[f'torch r={r}']) / med(t[f'augment r={r}']):.1f} x HIP | largest " \
                        f"byte difference HIP - torch {diff}"
            lines.append(line)
        k = "augment r=7 + out_f32"
        lines.append(f"  augment radius 7 with out_f32  HIP {span(t[k])} | derived floor {fl(27 * H * W):.1f} us ({27 * H * W / 1e6:.1f} MB) = "
                     f"{med(t[k]) * 1e3 / fl(27 * H * W):.1f} x")
        print("\n".join(lines[-7:]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--augment", action="store_true", help="time the background render and augment (DESIGN.md section 24) instead")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200, help="HIP calls per round")
    ap.add_argument("--torch-reps", type=int, default=10, help="calls of the torch restatement per round")
    ap.add_argument("--hip-only", action="store_true", help="time the HIP calls alone (for a kernel trace in a run of its own)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1080, 1920, 2160, 3840], help="height width pairs")
    ap.add_argument("--out", default=None, help="file the lines are written to (profiles/hsynth_bench.txt)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs the MI355X: nothing is measured without it"
    if args.augment:
        return bench_augment(args)
    lines = [f"woft_amd.hsynth on the device against torch ops on the device and the float64 numpy restatement on the host (+ upload); "
             f"{args.rounds} alternating rounds of {args.reps} HIP / {args.torch_reps} torch calls each (host: 1 call) after one warm-up round, "
             "per call through the public wrappers (allocation of the outputs and the host's 3x3 inversions included; back-to-back "
             "calls, the image may stay in the Infinity Cache): median (min - max); floors are DERIVED from the byte counts at the "
             "measured 6.29 TB/s, not measured"]
    for H, W in zip(args.sizes[0::2], args.sizes[1::2]):
        base = synth.make_template(H, W)
        base_d = torch.from_numpy(base).cuda()
        base_f = base_d.float()
        rs = np.random.RandomState(1)
        H_gt = random_homography(rs, H, W, 0.2)
        texs = [make_occluder(rs, 256, 320), make_occluder(rs, 192, 192)]
        place = lambda cx, cy, s: np.array([[s, 0, cx], [0, s, cy], [0, 0, 1.0]])
        occ_all = [(texs[0], place(0.2 * W, 0.3 * H, H / 1080.0) @ random_homography(rs, 256, 320, 0.2)),
                   (texs[1], place(0.5 * W, 0.4 * H, 1.5 * H / 1080.0) @ random_homography(rs, 192, 192, 0.2))]
        ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float64),
                                torch.arange(W, device="cuda", dtype=torch.float64), indexing="ij")
        for n_occ in (0, 2):
            occ = occ_all[:n_occ]
            occ_d = [(torch.from_numpy(t).cuda(), Ho) for t, Ho in occ]
            pre = []
            for t, Ho in occ_d:
                a = t[..., 3:].float() / 255
                pre.append((torch.cat([a * t[..., :3].float(), a], 2), torch.from_numpy(np.linalg.inv(Ho)).cuda()))
            Hinv, Hf = torch.from_numpy(np.linalg.inv(H_gt)).cuda(), torch.from_numpy(H_gt).cuda()
            gain, bias = 1.1, -5.0
            out = {}

            def hip_render():
                out["hip_r"] = render_pair(base_d, H_gt, occ_d, gain=gain, bias=bias)

            def hip_labels():
                out["hip_l"] = pair_labels((H, W), H_gt, occ_d)

            def t_render():
                out["t_r"] = torch_render(base_f, Hinv, gain, bias, pre, (xs, ys))[0]

            def t_labels():
                out["t_l"] = torch_labels(Hf, pre, (xs, ys), H, W)

            def np_render():
                v, _ = hsynth_host.render(base, H_gt, occ, gain, bias)
                out["np_r"] = torch.from_numpy(np.clip(np.rint(v), 0, 255).astype(np.uint8)).cuda()

            def np_labels():
                f, vis, ok = hsynth_host.labels((H, W), H_gt, occ)
                out["np_l"] = (torch.from_numpy(f.astype(np.float32)).cuda(), torch.from_numpy(vis.astype(np.float32)).cuda(),
                               torch.from_numpy(ok).cuda())

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            sides = [("hip_r", hip_render, args.reps), ("t_r", t_render, args.torch_reps), ("hip_l", hip_labels, args.reps),
                     ("t_l", t_labels, args.torch_reps)]
            if args.hip_only:
                sides = sides[0::2]
            t = {k: [] for k, _, _ in sides}
            for r in range(args.rounds + 1):
                for label, fn, reps in sides:
                    ms = _round(fn, reps)
                    if r > 0:
                        t[label].append(ms)
            if args.hip_only:
                lines.append(f"{H} x {W}, {n_occ} occluders: render_pair {sorted(t['hip_r'])[len(t['hip_r']) // 2] * 1e3:.1f} us, "
                             f"pair_labels {sorted(t['hip_l'])[len(t['hip_l']) // 2] * 1e3:.1f} us")
                print(lines[-1], flush=True)
                continue
            t["np_r"], t["np_l"] = [wall(np_render)], [wall(np_labels)]
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            diff_r = int((out["hip_r"].int() - out["t_r"].int()).abs().max())
            same_l = bool(torch.equal(out["hip_l"][1], out["t_l"][1]) and torch.equal(out["hip_l"][2], out["t_l"][2]))
            tex_bytes = sum(tt.size for tt, _ in occ)
            bytes_r = 3 * H * W * 2 + tex_bytes                      # the base read once, the frame written once, the textures
            bytes_l = (8 + 4 + 1) * H * W + tex_bytes                # flow, visible, valid written once
            span = lambda k, unit=1e3, u="us": f"{med[k] * unit:9.1f} {u} ({min(t[k]) * unit:.1f} - {max(t[k]) * unit:.1f})"
            fl = lambda b: b / (STREAM_TBPS * 1e12) * 1e6
            lines += [
                f"{H} x {W}, {n_occ} occluders",
                f"  render_pair  HIP {span('hip_r')} | derived floor {fl(bytes_r):.1f} us ({bytes_r / 1e6:.1f} MB) = "
                f"{med['hip_r'] * 1e3 / fl(bytes_r):.1f} x | torch ops {span('t_r')} = {med['t_r'] / med['hip_r']:.1f} x HIP | numpy + upload "
                f"{med['np_r']:.0f} ms | largest byte difference HIP - torch {diff_r}",
                f"  pair_labels  HIP {span('hip_l')} | derived floor {fl(bytes_l):.1f} us ({bytes_l / 1e6:.1f} MB) = "
                f"{med['hip_l'] * 1e3 / fl(bytes_l):.1f} x | torch ops {span('t_l')} = {med['t_l'] / med['hip_l']:.1f} x HIP | numpy + upload "
                f"{med['np_l']:.0f} ms | labels equal to torch's: {same_l}"]
            print("\n".join(lines[-3:]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
