"""What RAFT's video warm start costs and saves:

    python tools/bench_warm.py --out profiles/warm_start_bench.txt

(1) woft_forward_interpolate alone on the 1/8-resolution grids of 1080p (135 x 240) and 4K (270 x 480): HIP events around
    REPS back-to-back launches after a warm-up, the median of ROUNDS such measurements, on a smooth flow of a few cells plus noise.
    The figure to read it against is ONE refinement iteration (0.51 ms at 1080p, profiles/r06_layer_times_bf16x3.txt): warm start
    pays only if the interpolation costs less than the iterations it saves.
(2) a run of lost frames (every frame's re-detection verdict overruled, tools/bench_window.py's device) with the default tracker
    (WOFT.py) and with `warm_start_local` (WOFT_warmstart.py) at `warm_start_iters` = iters and iters / 2, in one process on
    identical frames: alternating rounds, host clock around work that ends in a device synchronise, min-max of the rounds next to
    the mean; the largest template-corner distance between the warm and the cold poses is reported, not judged (the synthetic
    checkpoint's flow is no motion estimate).
No GPU: the tool fails, it has no fallback."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.bench_window import SIZES, centred_mask, corners_gap, run  # noqa: E402

ROUNDS, FRAMES, WARMUP = 4, 24, 8
FI_REPS, FI_ROUNDS, FI_WARMUP = 20, 5, 5


def make_tracker(cfg, sd, iters, template, mask, **keys):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / cfg)
    conf.flow_config.model = sd
    conf.flow_config.iters = iters
    for k, v in keys.items():
        setattr(conf, k, v)
    trk = conf.tracker_class(conf)
    trk.init(template, mask)
    return trk


def bench_interpolate(say):
    from woft_amd import ops
    say(f"# woft_forward_interpolate: median over {FI_ROUNDS} measurements of {FI_REPS} back-to-back launches (HIP events) after "
        f"{FI_WARMUP} warm-up launches; smooth flow of a few cells + noise")
    say("# size | 1/8-resolution grid | points | ms per call (min-max of the measurements) | valid points")
    for sname, (H, W) in SIZES.items():
        hf, wf = H // 8, W // 8
        rs = np.random.RandomState(hf)
        ys, xs = np.mgrid[:hf, :wf]
        f = np.stack([3.0 * np.sin(xs / wf * 2.3) + 1.0, -2.0 * np.cos(ys / hf * 1.9)]) + rs.normal(0, 0.2, (2, hf, wf))
        flow = torch.from_numpy(f.astype(np.float32)).cuda()
        out = torch.empty_like(flow)
        for _ in range(FI_WARMUP):
            ops.forward_interpolate(flow, out)
        torch.cuda.synchronize()
        ms = []
        for _ in range(FI_ROUNDS):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(FI_REPS):
                ops.forward_interpolate(flow, out)
            e.record()
            e.synchronize()
            ms.append(s.elapsed_time(e) / FI_REPS)
        x1, y1 = xs + f[0], ys + f[1]
        valid = int(((x1 > 0) & (x1 < wf) & (y1 > 0) & (y1 < hf)).sum())
        say(f"{sname} | {hf} x {wf} | {hf * wf} | {np.median(ms):.4f} ms ({min(ms):.4f}-{max(ms):.4f}) | {valid}")


def bench_trackers(args, say):
    import bench
    from woft_amd import synth
    sd = synth.make_state_dict(seed=7)
    half = max(1, args.iters // 2)
    say(f"# lost-frame runs: {ROUNDS} alternating rounds x {FRAMES} frames per tracker after {WARMUP} warm-up frames each, every "
        f"frame's re-detection overruled; {args.iters} flow iterations; device {torch.cuda.get_device_name(0)}")
    say("# size | tracker: frames/s (min-max of the rounds) ms/frame | ... | ratios to cold | warm-started frames of the last "
        "round | largest template-corner distance to the cold poses in the last round [px]")
    for sname in args.sizes:
        H, W = SIZES[sname]
        template, frames = bench.make_sequence(H, W, 0, bench.CLIP)
        mask = centred_mask(H, W, 2)
        trackers = [("cold", make_tracker("WOFT.py", sd, args.iters, template, mask)),
                    (f"warm it{args.iters}", make_tracker("WOFT_warmstart.py", sd, args.iters, template, mask)),
                    (f"warm it{half}", make_tracker("WOFT_warmstart.py", sd, args.iters, template, mask, warm_start_iters=half))]
        for _, trk in trackers:
            run(trk, frames, 0, WARMUP, force_lost=True)
        fps = {tag: [] for tag, _ in trackers}
        res = {}
        for r in range(ROUNDS):
            first = WARMUP + r * FRAMES
            k = r % len(trackers)
            for tag, trk in trackers[k:] + trackers[:k]:
                if first % bench.CLIP:                     # every tracker starts a round from the same pose: the clip's, restarted
                    bench.restart_clip(trk)
                trk._warm = None
                dt, res[tag] = run(trk, frames, first, FRAMES, force_lost=True)
                fps[tag].append(FRAMES / dt)
        cold = np.array(fps["cold"])
        parts, ratios, extra = [], [], []
        for tag, _ in trackers:
            v = np.array(fps[tag])
            parts.append(f"{tag} {v.mean():7.1f} fps ({v.min():.1f}-{v.max():.1f}) {1000 / v.mean():6.2f} ms")
            if tag != "cold":
                ratios.append(f"x{v.mean() / cold.mean():.3f}")
                n_warm = sum(int(m.local_warm_started) for _, m in res[tag])
                gap = max(corners_gap(Hw, Hc, mask) for (Hw, _), (Hc, _) in zip(res[tag], res["cold"]))
                extra.append(f"{n_warm} of {FRAMES}, {gap:.3f} px")
        say(f"{sname} | " + " | ".join(parts) + " | " + " ".join(ratios) + " | " + " ; ".join(extra))
        del trackers
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=["1080p"], choices=list(SIZES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_warm.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/bench_warm.py on {torch.cuda.get_device_name(0)}")
    bench_interpolate(say)
    bench_trackers(args, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
