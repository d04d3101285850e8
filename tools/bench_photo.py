"""Times of the photometric refinement (woft_amd.photo, csrc/photo.hip) at 1080p and 4K with a centred
quarter-frame mask:

    python tools/bench_photo.py --out profiles/photo_refine_bench.txt

  * one single evaluation (the accumulate launch and its one-workgroup sum launch) at strides 1 and 2, device events around REPS
    calls, against its streaming floor -- DERIVED: the bytes of the template, mask and frame pixels under the mask's box, from the
    shapes, over the 6.29 TB/s this project measured for a streaming kernel; not a measurement;
  * one 10-iteration refinement including its one read (host clock around PhotoTemplate.refine, which ends in an event
    synchronise), with the default eps (it may stop early: the evaluated iterates are printed) and with eps = 0 (all 11);
  * the tracker of WOFT.py against WOFT_photo.py in one process on identical frames, alternating rounds in the style of
    tools/bench_window.py.  The synthetic checkpoint's flow is no motion estimate, so besides the trackers as they are (the
    refined-frame count says how often the stage ran at all) a second pair of lines overrules every frame's global fit in BOTH
    trackers with the sequence's own pose, its box corners moved by up to 1 px: the flow still runs, the re-detection succeeds,
    and the refinement starts from a pose as a trained network would leave it.
No GPU: the tool fails, it has no fallback."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ROUNDS, FRAMES, WARMUP, REPS = 3, 16, 6, 50
SIZES = {"1080p": (1080, 1920), "4K": (2160, 3840)}
STREAM_BYTES_PER_S = 6.29e12


def centred_mask(H, W, k=2):
    m = np.zeros((H, W), np.uint8)
    h, w = H // k, W // k
    m[(H - h) // 2:(H - h) // 2 + h, (W - w) // 2:(W - w) // 2 + w] = 255
    return m


def perturbed(Hm, box, rs, px=1.0):
    """Hm with the images of the box's corners moved by up to px."""
    from woft_amd.hsynth import homography_from_4pts
    x0, y0, x1, y1 = box
    c = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)
    q = Hm @ np.concatenate([c, np.ones((4, 1))], 1).T
    return homography_from_4pts(c, (q[:2] / q[2]).T + rs.uniform(-px, px, (4, 2)))


def bench_kernels(sname, template, mask, frame, W0, say):
    from woft_amd import ops
    from woft_amd.photo import PhotoTemplate
    for stride in (1, 2):
        pt = PhotoTemplate(template, mask, stride=stride)
        out = torch.empty(ops.PHOTO_NACC, dtype=torch.float64, device="cuda")
        call = lambda: ops.photo_eval(pt.template, pt.mask, None, frame, pt.box, stride, W0, 1.0, 0.0, True, None, out)
        for _ in range(5):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            call()
        e1.record()
        torch.cuda.synchronize()
        us = 1000.0 * e0.elapsed_time(e1) / REPS
        n_box = (pt.box[2] - pt.box[0] + 1) * (pt.box[3] - pt.box[1] + 1)
        n_part = -(-(((pt.box[2] - pt.box[0]) // stride + 1) * ((pt.box[3] - pt.box[1]) // stride + 1)) // ops.PHOTO_CHUNK)
        nbytes = n_box * (3 + 1 + 3)          # template, mask and frame pixels under the box (every row and line is touched at stride 2 too)
        floor_us = 1e6 * nbytes / STREAM_BYTES_PER_S
        say(f"{sname} | single evaluation, stride {stride}: {us:8.1f} us per call (accumulate + sum launch, {REPS} calls between device "
            f"events), n_set {pt.n_set}, partials {n_part} | streaming floor DERIVED from shapes: "
            f"{nbytes / 1e6:.2f} MB / 6.29 TB/s = {floor_us:.2f} us | x{us / floor_us:.1f} of the floor")
    pt = PhotoTemplate(template, mask)
    for eps, label in ((1e-3, "default eps 1e-3"), (0.0, "eps 0")):
        for _ in range(3):
            H, info = pt.refine(frame, W0, iters=10, eps=eps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            H, info = pt.refine(frame, W0, iters=10, eps=eps)
        ms = 1000.0 * (time.perf_counter() - t0) / REPS
        say(f"{sname} | refinement, 10 iterations, {label}: {ms:7.3f} ms per call including its read (host clock, {REPS} calls), "
            f"{info.status} after {len(info.cost)} evaluated iterates, cost {info.rms_before:.2f} -> {info.rms_after:.2f}")


def make_tracker(cfg, sd, iters, template, mask):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / cfg)
    conf.flow_config.model = sd
    conf.flow_config.iters = iters
    trk = conf.tracker_class(conf)
    trk.init(template, mask)
    return trk


def run(trk, frames, first, n, poses=None):
    """-> (seconds, results) for frames[first : first + n] of the clip; poses: frame index -> the pose (frame -> template) that
    replaces the global fit's, with a successful verdict (the flow and the fit still run)."""
    import bench
    inner = type(trk)._global_stage.__get__(trk)
    at = {"i": first}

    def overruled(frame, prewarp_H):
        fit = inner(frame, prewarp_H)
        fit.H = poses[at["i"] % bench.CLIP] @ np.linalg.inv(prewarp_H)
        fit.success = True
        return fit
    if poses is not None:
        trk._global_stage = overruled
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = []
    for i in range(first, first + n):
        if i % bench.CLIP == 0:
            bench.restart_clip(trk)
        at["i"] = i
        res.append(trk.track(frames[i % bench.CLIP]))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if poses is not None:
        del trk._global_stage
    return dt, res


def bench_trackers(sname, template, mask, frames, poses, iters, say):
    import bench
    from woft_amd import synth
    sd = synth.make_state_dict(seed=7)
    plain = make_tracker("WOFT.py", sd, iters, template, mask)
    photo = make_tracker("WOFT_photo.py", sd, iters, template, mask)
    for label, ps in (("trackers as they are", None), ("global fit overruled with the sequence's pose, corners moved by <= 1 px", poses)):
        for trk in (plain, photo):
            bench.restart_clip(trk)
            run(trk, frames, 0, WARMUP, ps)
        fps = {"plain": [], "photo": []}
        refined = evaluated = 0
        for r in range(ROUNDS):
            first = WARMUP + r * FRAMES
            order = (("plain", plain), ("photo", photo)) if r % 2 == 0 else (("photo", photo), ("plain", plain))
            for tag, trk in order:
                bench.restart_clip(trk)
                dt, res = run(trk, frames, first, FRAMES, ps)
                fps[tag].append(FRAMES / dt)
                if tag == "photo":
                    done = [m.photo for _, m in res if getattr(m, "photo", None) is not None]
                    refined += len(done)
                    evaluated += sum(p.iterates for p in done)
        a, b = np.array(fps["plain"]), np.array(fps["photo"])
        say(f"{sname} | {label} | WOFT {1000 / a.mean():6.2f} ms/frame ({a.min():.1f}-{a.max():.1f} fps) | WOFT_photo "
            f"{1000 / b.mean():6.2f} ms/frame ({b.min():.1f}-{b.max():.1f} fps) | difference {1000 / b.mean() - 1000 / a.mean():+.3f} ms | "
            f"refined {refined} of {ROUNDS * FRAMES} frames, {evaluated / max(refined, 1):.1f} evaluated iterates per refined frame")
    del plain, photo
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trackers", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_photo.py needs a GPU")
    import bench
    from woft_amd import synth
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/bench_photo.py: device {torch.cuda.get_device_name(0)}; quarter-frame centred mask; trackers: {ROUNDS} alternating "
        f"rounds x {FRAMES} frames after {WARMUP} warm-up frames each, {args.iters} flow iterations, seeded random weights")
    for sname in args.sizes:
        H, W = SIZES[sname]
        template, frames = bench.make_sequence(H, W, 0, bench.CLIP)
        mask = centred_mask(H, W)
        ys, xs = np.nonzero(mask)
        box = (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))
        rs = np.random.RandomState(17)
        true = [synth.seq_homography(t, H, W) for t in range(1, bench.CLIP + 1)]            # template -> frame
        bench_kernels(sname, template, mask, frames[2], perturbed(true[2], box, rs), say)
        if not args.no_trackers:
            poses = [np.linalg.inv(perturbed(Ht, box, rs)) for Ht in true]                   # frame -> template
            bench_trackers(sname, template, mask, frames, poses, args.iters, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
