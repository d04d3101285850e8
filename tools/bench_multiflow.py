"""What the candidate fold and the multi-delta tracker cost:

    python tools/bench_multiflow.py --out profiles/multiflow_bench.txt

(1) woft_flow_chain_fold at 1080p and 4K, in one process: HIP events around REPS back-to-back launches after a warm-up, the median
    of ROUNDS such measurements, alternating with the same arithmetic from existing ops (ops.flow_chain for the flow, a torch
    restatement of the edge-exact sampler for the logits, torch elementwise passes for cost, visibility and the selection), next to
    the streaming floor: the bytes the launch must move, counted from its arguments by `fold_bytes`, over the HBM rate measured
    on this part by tools/bench_flow_chain.py (6.29 TB/s).  Three forms: a null-prev candidate that starts a fold, a full
    candidate that starts a fold (every pixel written), a full candidate folded into a best it does not beat (the steady state
    of back-to-back launches on one buffer set: the best is read, nothing is written).  Every launch works on another of N buffer
    sets that together exceed the 256 MiB Infinity Cache.
(2) MultiFlowTracker.track per frame for deltas (None,), (None, 1) and the default seven, on the synthetic checkpoint: host clock
    around FRAMES frames that end in a device synchronise, after a warm-up long enough for every delta to have a source frame,
    alternating rounds.
No GPU: the tool fails, it has no fallback."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.bench_flow_chain import CACHE_BYTES, HBM_MEASURED, K_REPS, K_ROUNDS, K_WARMUP, smooth_flow, torch_landing  # noqa: E402
from tools.bench_window import SIZES  # noqa: E402

ROUNDS, FRAMES = 3, 12
DELTAS = ((None,), (None, 1), (None, 1, 2, 4, 8, 16, 32))


def fold_bytes(prev, wlogit, mlogit, first, replaced):
    """Bytes per pixel one fold launch must move: the prev planes (flow x 2, cost, vis) and the step planes (flow x 2 and each
    logit given) read once; of the running best, sel, cost and vis read unless `first` (its flow is never read) and all five planes
    written where the candidate replaces it (`replaced`: the share of such pixels, 1 with `first`)."""
    read = (4 if prev else 0) + 2 + bool(wlogit) + bool(mlogit) + (0 if first else 3)
    return 4 * (read + 5 * (1.0 if first else replaced))


def torch_sample_planes(f, qx, qy):
    """The edge-exact sampler on (C, h, w) in torch ops (fp32), at points already clamped into the plane."""
    c, h, w = f.shape
    x0, y0 = qx.floor().clamp(0, w - 1), qy.floor().clamp(0, h - 1)
    ax, ay = qx - x0, qy - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    flat = f.reshape(c, -1)
    g = lambda yy, xx: flat[:, (yy * w + xx).reshape(-1)].reshape(c, h, w)
    return (1 - ay) * ((1 - ax) * g(y0, x0) + ax * g(y0, x1)) + ay * ((1 - ax) * g(y1, x0) + ax * g(y1, x1))


def fold_by_existing_ops(best, prev, sflow, logits, k, thr, first):
    """The fold from what the tree had before: woft_flow_chain, the sampler in torch, torch elementwise passes."""
    from woft_amd import ops
    pflow, pcost, pvis = prev
    flow = ops.flow_chain(pflow, sflow)
    qx, qy, valid = torch_landing(pflow)
    l = torch_sample_planes(logits, qx, qy)
    cost = pcost + torch.nn.functional.softplus(-l[0])
    vis = pvis * torch.sigmoid(l[1])
    ok = valid & torch.isfinite(flow).all(0) & torch.isfinite(cost) & torch.isfinite(vis)
    bf, bc, bv, bs = best
    if first:
        replace = ok
    else:
        occ, bocc = vis < thr, bv < thr
        replace = ok & ((bs < 0) | (bocc & ~occ) | ((bocc == occ) & (cost < bc)))
    return (torch.where(replace, flow, bf), torch.where(replace, cost, bc), torch.where(replace, vis, bv),
            torch.where(replace, torch.full_like(bs, k), bs))


def timed_pair(fns, n_sets):
    """Median (min, max) ms per call of each function, measured in alternating rounds."""
    for fn in fns:
        for i in range(K_WARMUP):
            fn(i % n_sets)
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(K_ROUNDS):
        for j, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(K_REPS):
                fn(i % n_sets)
            e.record()
            e.synchronize()
            ms[j].append(s.elapsed_time(e) / K_REPS)
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def bench_kernels(say):
    from woft_amd import ops
    say(f"# fold: median over {K_ROUNDS} alternating measurements of {K_REPS} back-to-back calls (HIP events) after {K_WARMUP} warm-up "
        f"calls, rotating over buffer sets of >= {CACHE_BYTES >> 20} MiB in all; floor = bytes / {HBM_MEASURED / 1e12:.2f} TB/s")
    say("# size | form | woft_flow_chain_fold ms (min-max) | existing ops ms (min-max) | floor ms (bytes per pixel) | fold / floor | "
        "existing ops / fold")
    for sname, (h, w) in SIZES.items():
        n = h * w
        n_sets = max(2, -(-CACHE_BYTES // (n * 52)))
        plane = lambda lo, hi, seed: (lo + (hi - lo) * torch.rand(h, w, device="cuda",
                                                                  generator=torch.Generator(device="cuda").manual_seed(seed)))
        pflow = [smooth_flow(h, w, 10 + i, 1.0) for i in range(n_sets)]
        sflow = [smooth_flow(h, w, 50 + i, -1.0) for i in range(n_sets)]
        pcost, pvis = [plane(1.0, 2.0, 90 + i) for i in range(n_sets)], [plane(0.6, 1.0, 130 + i) for i in range(n_sets)]
        logits = [torch.stack([plane(2.0, 4.0, 170 + i), plane(2.0, 4.0, 210 + i)]) for i in range(n_sets)]
        new_best = lambda: [(torch.empty(2, h, w, device="cuda"), torch.empty(h, w, device="cuda"), torch.empty(h, w, device="cuda"),
                             torch.empty(h, w, dtype=torch.int32, device="cuda")) for _ in range(n_sets)]
        best = new_best()
        prev = [(pflow[i], pcost[i], pvis[i]) for i in range(n_sets)]

        def fold(i, with_prev, first, k):
            ops.flow_chain_fold(best[i], prev[i] if with_prev else None, sflow[i], logits[i][0], logits[i][1], k=k, first=first)
        identity = (torch.zeros(2, h, w, device="cuda"), torch.zeros(h, w, device="cuda"), torch.ones(h, w, device="cuda"))
        rows = [("null prev, first", fold_bytes(False, True, True, True, 1.0), lambda i: fold(i, False, True, 0),
                 lambda i: fold_by_existing_ops(best[i], identity, sflow[i], logits[i], 0, 0.5, True)),
                ("full candidate, first", fold_bytes(True, True, True, True, 1.0), lambda i: fold(i, True, True, 1),
                 lambda i: fold_by_existing_ops(best[i], prev[i], sflow[i], logits[i], 1, 0.5, True)),
                # (after the rows above every best holds this very candidate: an equal key replaces nothing)
                ("full candidate into a best it does not beat", fold_bytes(True, True, True, False, 0.0),
                 lambda i: fold(i, True, False, 2), lambda i: fold_by_existing_ops(best[i], prev[i], sflow[i], logits[i], 2, 0.5, False))]
        for name, bpp, fn, ref in rows:
            k, t = timed_pair((fn, ref), n_sets)
            floor = n * bpp / HBM_MEASURED * 1e3
            say(f"{sname} | {name} | {k[0]:.4f} ({k[1]:.4f}-{k[2]:.4f}) | {t[0]:.4f} ({t[1]:.4f}-{t[2]:.4f}) | {floor:.4f} ({bpp:.0f} B) | "
                f"x{k[0] / floor:.2f} | x{t[0] / k[0]:.1f}")
        del pflow, sflow, pcost, pvis, logits, best, prev, identity
        torch.cuda.empty_cache()


def bench_trackers(args, say):
    import bench
    from pytracking.utils.config import load_config
    from woft_amd import MultiFlowTracker, synth
    sd = synth.make_state_dict(seed=7)
    warm = max(d for d in DELTAS[-1] if d is not None) + 2
    say(f"# MultiFlowTracker.track: {ROUNDS} alternating rounds x {FRAMES} frames per tracker after {warm} warm-up frames each (every "
        f"delta has its source frame); raft_type 'weighted', {args.iters} flow iterations; host clock, one synchronise per round")
    say("# size | per deltas: ms per frame (min-max of the rounds), flows per frame | ms per frame over that of deltas=(None,)")
    for sname in args.sizes:
        H, W = SIZES[sname]
        _, frames = bench.make_sequence(H, W, 0, bench.CLIP)
        trackers = []
        for deltas in DELTAS:
            fc = load_config(ROOT / "pytracking" / "optical_flow" / "configs" / "v2_SNOB_large_g05_RAFT.py")
            fc.model, fc.iters = sd, args.iters
            trk = MultiFlowTracker(fc.of_class(fc), deltas=deltas)
            trk.init(frames[0])
            for t in range(1, warm + 1):
                trk.track(frames[t % len(frames)])
            trackers.append((deltas, trk))
        torch.cuda.synchronize()
        ms = {d: [] for d in DELTAS}
        for r in range(ROUNDS):
            k = r % len(trackers)
            for deltas, trk in trackers[k:] + trackers[:k]:
                t0 = time.perf_counter()
                for _ in range(FRAMES):
                    trk.track(frames[(trk.frame_index + 1) % len(frames)])
                torch.cuda.synchronize()
                ms[deltas].append((time.perf_counter() - t0) / FRAMES * 1e3)
        base = float(np.mean(ms[DELTAS[0]]))
        say(f"{sname} | " + " | ".join(f"{d!r}: {np.mean(ms[d]):.2f} ms ({min(ms[d]):.2f}-{max(ms[d]):.2f}), {len(d)} flows"
                                      for d in DELTAS) + " | " + " ".join(f"x{np.mean(ms[d]) / base:.2f}" for d in DELTAS[1:]))
        del trackers
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_multiflow.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/bench_multiflow.py on {torch.cuda.get_device_name(0)}")
    bench_kernels(say)
    bench_trackers(args, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
