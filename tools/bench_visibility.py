"""Frames/s of the full-frame tracker with the MaskHead's visibility mask consumed (pytracking/configs/WOFT_visibility.py:
'weighted_masked' network, visibility_mode 'gate') against the default tracker (WOFT.py) on identical frames, in one process:

    python tools/bench_visibility.py --out profiles/visibility_bench.txt

The sequences are bench.py's (woft_amd.synth, shipped arithmetic, 12 flow iterations), the mask a centred rectangle covering 1/4 of
the frame; the synthetic checkpoint is the same for both but for the mask head's tensors (drawn last).  Both trackers are warmed up,
then timed in ROUNDS alternating rounds of FRAMES frames each (host clock around work that ends in a device synchronise), the form
of tools/bench_window.py: clock drift and neighbours on the host hit both, and the spread of the rounds is printed next to the mean.
Seeded random weights give an arbitrary mask, so the gate's threshold is the median visibility of the template pixels in one flow
(about half of the correspondences survive); --mode weight times the other rule.  No GPU: the tool fails, it has no fallback."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.bench_window import SIZES, centred_mask, run  # noqa: E402

ROUNDS, FRAMES, WARMUP = 4, 24, 8
STRUCTURE = [(128, 3), (128, 3)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=["1080p"], choices=list(SIZES))
    ap.add_argument("--mode", default="gate", choices=["gate", "weight"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_visibility.py needs a GPU")
    import bench
    from woft_amd import synth
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    sd_plain = synth.make_state_dict(seed=7)
    sd_mask = synth.make_state_dict(seed=7, mask_head_structure=STRUCTURE)
    say(f"# tools/bench_visibility.py: {ROUNDS} alternating rounds x {FRAMES} frames per tracker after {WARMUP} warm-up frames each; "
        f"{args.iters} flow iterations; visibility_mode '{args.mode}'; mask head {STRUCTURE}; device {torch.cuda.get_device_name(0)}")
    say("# size | WOFT: frames/s (min-max of the rounds) ms/frame | WOFT_visibility: the same | ratio | threshold | "
        "kept after masks and gate (mean of the last round) | lost frames in the last round WOFT / WOFT_visibility")
    for sname in args.sizes:
        H, W = SIZES[sname]
        template, frames = bench.make_sequence(H, W, 0, bench.CLIP)
        mask = centred_mask(H, W, 2)
        base = make_tracker("WOFT.py", sd_plain, args.iters, template, mask)
        probe = make_tracker("WOFT_visibility.py", sd_mask, args.iters, template, mask)
        p = probe.flower.compute_flow(template, frames[0], mode="TC", do_sigmoid=True, visibility=True)[3]
        thr = float(np.float32(np.median(p.cpu().numpy().reshape(-1)[mask.reshape(-1) > 0])))
        thr = min(max(thr, 1e-6), 1.0 - 1e-6)
        del probe
        vis = make_tracker("WOFT_visibility.py", sd_mask, args.iters, template, mask, visibility_mode=args.mode, visibility_thr=thr)
        run(base, frames, 0, WARMUP)
        run(vis, frames, 0, WARMUP)
        fps = {"base": [], "vis": []}
        for r in range(ROUNDS):
            first = WARMUP + r * FRAMES
            order = (("base", base), ("vis", vis)) if r % 2 == 0 else (("vis", vis), ("base", base))
            res = {}
            for tag, trk in order:
                if first % bench.CLIP:                     # both start a round from the same pose: the clip's, restarted
                    bench.restart_clip(trk)
                dt, res[tag] = run(trk, frames, first, FRAMES)
                fps[tag].append(FRAMES / dt)
        b, v = np.array(fps["base"]), np.array(fps["vis"])
        kept = np.mean([m.n_kept for _, m in res["vis"]])
        lost = sum(int(m.lost) for _, m in res["base"]), sum(int(m.lost) for _, m in res["vis"])
        say(f"{sname} | WOFT {b.mean():7.1f} fps ({b.min():.1f}-{b.max():.1f}) {1000 / b.mean():6.2f} ms | WOFT_visibility "
            f"{v.mean():7.1f} fps ({v.min():.1f}-{v.max():.1f}) {1000 / v.mean():6.2f} ms | x{v.mean() / b.mean():.3f} | thr {thr:.6f} | "
            f"{kept:.0f} of {int((mask > 0).sum())} | {lost[0]} / {lost[1]}")
        del base, vis
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
