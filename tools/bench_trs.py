#!/usr/bin/env python
"""RANSAC similarity (csrc/trs.hip) on MI355X: fit time per call against the RANSAC homography (csrc/ransac.hip) in the same
process on the same points, and tracked frames/s of the WOFT_TRS config against WOFT_RANSAC and the default WOFT config.

  python tools/bench_trs.py [--steps K] [--warmup W] [--rounds R] [--fits-only] [--n N ...]

Fits: N correspondences (default 500) of a known similarity plus N(0, 0.5) px noise and 0 / 30 / 60 % outliers, max_iters 10000,
threshold 3 px, each estimator at its preset's confidence (TRS 0.999, RANSAC 0.995); per estimator W warm-up calls, then R rounds
of K calls between two HIP events (device time per call, launches included), the two estimators alternated round by round
(T R T R ...) to spread any drift of the box over both -- the mean and the range of the rounds are printed, with the iterations
the adaptive stop ran and the inliers found.
Tracker: 1080p, 12 RAFT iterations, synthetic sequence and checkpoint of bench.py (make_sequence / restart_clip), W warm-up and K
timed track() calls per config, the three configs alternated twice (A B C A B C).  With random flow weights the estimated poses
are meaningless (bench.py's note); the lost-frame count of each run is printed because a lost frame costs a second flow.
Prints a table and one JSON line."""
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

_ANG = np.deg2rad(3.0)
S_TRUE = np.array([[1.05 * np.cos(_ANG), -1.05 * np.sin(_ANG), 12.0], [1.05 * np.sin(_ANG), 1.05 * np.cos(_ANG), -7.0]])


def points(n, outliers, seed, w=1920, h=1080):
    rng = np.random.default_rng(seed)
    a = rng.random((n, 2)) * [w, h]
    b = np.c_[a, np.ones(n)] @ S_TRUE.T + rng.normal(0.0, 0.5, (n, 2))
    out = rng.permutation(n)[:int(round(outliers * n))]
    ang = rng.random(out.size) * 2 * np.pi
    b[out] += np.c_[np.cos(ang), np.sin(ang)] * (20.0 + 40.0 * rng.random(out.size))[:, None]
    return torch.from_numpy(a.astype(np.float32)).cuda(), torch.from_numpy(b.astype(np.float32)).cuda()


def bench_fits(steps, warmup, rounds, sizes):
    rows = []
    max_iters = 10000
    for n in sizes:
        for outl in (0.0, 0.3, 0.6):
            a, b = points(n, outl, seed=n + int(100 * outl))
            Hout = torch.empty(9, device="cuda")
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
            info = torch.zeros(3, dtype=torch.int32, device="cuda")
            fits = dict(trs=lambda ws: ops.trs(a, b, Hout, st, max_iters=max_iters, thr=3.0, conf=0.999, info=info, ws=ws),
                        ransac=lambda ws: ops.ransac(a, b, Hout, st, max_iters=max_iters, thr=3.0, conf=0.995, info=info, ws=ws))
            wss = dict(trs=ops.trs_ws(n, max_iters), ransac=ops.ransac_ws(n, max_iters))
            us = dict(trs=[], ransac=[])
            infos = {}
            for name, fit in fits.items():
                for _ in range(warmup):
                    fit(wss[name])
            for _ in range(rounds):
                for name, fit in fits.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(steps):
                        fit(wss[name])
                    e1.record()
                    torch.cuda.synchronize()
                    us[name].append(e0.elapsed_time(e1) * 1e3 / steps)
                    infos[name] = info.cpu().tolist() + [int(st.item())]
            for name in fits:
                i, t = infos[name], us[name]
                rows.append(dict(estimator=name, n=n, outliers=outl, max_iters=max_iters, us_per_fit=round(float(np.mean(t)), 1),
                                 us_min=round(min(t), 1), us_max=round(max(t), 1), status=i[3], inliers=i[0], best_k=i[1],
                                 iterations=i[2], calls=steps * rounds))
                print(f"fit  {name:6s}  N={n:8d}  outliers={outl:3.1f}  max_iters={max_iters:5d}  {np.mean(t):8.1f} us/fit  "
                      f"(rounds {min(t):.1f} .. {max(t):.1f}; iterations run {i[2]:5d}, inliers {i[0]}, status {i[3]})", flush=True)
    return rows


def bench_tracker(steps, warmup):
    import bench
    from pytracking.utils.config import load_config
    from woft_amd import synth
    H, W, iters = 1080, 1920, 12
    sd = synth.make_state_dict(seed=7)
    template, frames = bench.make_sequence(H, W, 0, bench.CLIP)
    mask = synth.make_init_mask(H, W)
    names = ("WOFT", "WOFT_RANSAC", "WOFT_TRS")
    trackers = {}
    for name in names:
        conf = load_config(ROOT / "pytracking" / "configs" / (name + ".py"))
        conf.flow_config.model = sd
        conf.flow_config.iters = iters
        trk = conf.tracker_class(conf)
        trk.init(template, mask)
        assert trk._fused is not None, trk.solver_decision
        trackers[name] = trk
    res = {name: dict(seconds=0.0, frames=0, lost=0) for name in names}
    for name in names + names:
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
    out["trs_vs_ransac"] = round(out["WOFT_TRS"]["frames_per_s"] / out["WOFT_RANSAC"]["frames_per_s"], 4)
    out["trs_vs_wlsq"] = round(out["WOFT_TRS"]["frames_per_s"] / out["WOFT"]["frames_per_s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4, help="timed rounds per estimator and fit row, alternated")
    ap.add_argument("--fits-only", action="store_true")
    ap.add_argument("--n", type=int, nargs="+", default=[500], help="numbers of correspondences of the fit rows")
    args = ap.parse_args()
    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, rounds=args.rounds,
                  fits=bench_fits(args.steps, args.warmup, args.rounds, args.n))
    if not args.fits_only:
        result["tracker_1080p_12it"] = bench_tracker(args.steps, args.warmup)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
