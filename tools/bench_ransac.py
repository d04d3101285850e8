#!/usr/bin/env python
"""RANSAC homography (csrc/ransac.hip) on MI355X: fit time per call, and tracked frames/s of the WOFT_RANSAC config against
the default WOFT config in the same process.

  python tools/bench_ransac.py [--steps K] [--warmup W] [--fits-only] [--n N ...]

Fits: N in {4, 500, 4096, 1920*1080} correspondences of a known homography plus 0 / 30 / 60 % outliers, max_iters 10000
(200 for the full frame), threshold 3 px, confidence 0.995; W warm-up calls, then K calls between two HIP events (device time
per call, launches included) -- the iterations the adaptive stop ran and the inliers found are printed with each row.
Tracker: 1080p, 12 RAFT iterations, synthetic sequence and checkpoint of bench.py (make_sequence / restart_clip), W warm-up
and K timed track() calls per config, the two configs alternated twice (A B A B) to spread any drift of the box over both.
With random flow weights the estimated poses are meaningless (bench.py's note); the lost-frame count of each run is printed
because a lost frame costs a second flow.  Prints a table and one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np
import torch

from woft_amd import ops

H_TRUE = np.array([[1.03, 0.04, 12.0], [-0.03, 0.97, -7.0], [1.2e-4, -8e-5, 1.0]])


def points(n, outliers, seed, w=1920, h=1080):
    rng = np.random.default_rng(seed)
    a = rng.random((n, 2)) * [w, h]
    q = np.c_[a, np.ones(n)] @ H_TRUE.T
    b = q[:, :2] / q[:, 2:] + rng.normal(0.0, 0.5, (n, 2))
    out = rng.permutation(n)[:int(round(outliers * n))]
    ang = rng.random(out.size) * 2 * np.pi
    b[out] += np.c_[np.cos(ang), np.sin(ang)] * (20.0 + 40.0 * rng.random(out.size))[:, None]
    return torch.from_numpy(a.astype(np.float32)).cuda(), torch.from_numpy(b.astype(np.float32)).cuda()


def bench_fits(steps, warmup, sizes):
    rows = []
    for n in sizes:
        max_iters = 200 if n > 100000 else 10000
        for outl in ((0.0,) if n == 4 else (0.0, 0.3, 0.6)):
            a, b = points(n, outl, seed=n + int(100 * outl))
            Hout = torch.empty(9, device="cuda")
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
            info = torch.zeros(3, dtype=torch.int32, device="cuda")
            ws = ops.ransac_ws(n, max_iters)
            k = steps if n < 100000 else max(1, min(steps, 20))
            for _ in range(warmup):
                ops.ransac(a, b, Hout, st, max_iters=max_iters, thr=3.0, conf=0.995, info=info, ws=ws)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(k):
                ops.ransac(a, b, Hout, st, max_iters=max_iters, thr=3.0, conf=0.995, info=info, ws=ws)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / k
            i = info.cpu().tolist()
            rows.append(dict(n=n, outliers=outl, max_iters=max_iters, us_per_fit=round(us, 1), status=int(st.item()),
                             inliers=i[0], best_k=i[1], iterations=i[2], calls=k))
            print(f"fit  N={n:8d}  outliers={outl:3.1f}  max_iters={max_iters:5d}  {us:10.1f} us/fit  "
                  f"(iterations run {i[2]:5d}, inliers {i[0]}, status {int(st.item())})", flush=True)
    return rows


def bench_tracker(steps, warmup):
    import bench
    from pytracking.utils.config import load_config
    from woft_amd import synth
    H, W, iters = 1080, 1920, 12
    sd = synth.make_state_dict(seed=7)
    template, frames = bench.make_sequence(H, W, 0, bench.CLIP)
    mask = synth.make_init_mask(H, W)
    trackers = {}
    for name in ("WOFT", "WOFT_RANSAC"):
        conf = load_config(ROOT / "pytracking" / "configs" / (name + ".py"))
        conf.flow_config.model = sd
        conf.flow_config.iters = iters
        trk = conf.tracker_class(conf)
        trk.init(template, mask)
        assert trk._fused is not None, trk.solver_decision
        trackers[name] = trk
    res = {name: dict(seconds=0.0, frames=0, lost=0) for name in trackers}
    for name in ("WOFT", "WOFT_RANSAC", "WOFT", "WOFT_RANSAC"):
        trk = trackers[name]
        bench.restart_clip(trk)
        for i in range(warmup):
            trk.track(frames[i % bench.CLIP])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lost = 0
        for i in range(warmup, warmup + steps):
            if i % bench.CLIP == 0:
                bench.restart_clip(trk)
            _, meta = trk.track(frames[i % bench.CLIP])
            lost += int(meta.lost)
        torch.cuda.synchronize()
        r = res[name]
        r["seconds"] += time.perf_counter() - t0
        r["frames"] += steps
        r["lost"] += lost
    out = {}
    for name, r in res.items():
        fps = r["frames"] / r["seconds"]
        out[name] = dict(frames_per_s=round(fps, 2), frames=r["frames"], lost_frames=r["lost"])
        print(f"track  {name:12s}  {fps:7.2f} frames/s  ({r['frames']} frames, {r['lost']} lost)", flush=True)
    out["ransac_vs_wlsq"] = round(out["WOFT_RANSAC"]["frames_per_s"] / out["WOFT"]["frames_per_s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fits-only", action="store_true")
    ap.add_argument("--n", type=int, nargs="+", default=[4, 500, 4096, 1920 * 1080],
                    help="numbers of correspondences of the fit rows (e.g. --n 500 for a kernel table of that size alone)")
    args = ap.parse_args()
    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
                  fits=bench_fits(args.steps, args.warmup, args.n))
    if not args.fits_only:
        result["tracker_1080p_12it"] = bench_tracker(args.steps, args.warmup)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
