"""What the step from a fold result to the planar fit's correspondences, and the planar tracker on chained flow, cost (DESIGN.md
section 19):

    python tools/bench_chained.py --out profiles/chained_bench.txt

(1) woft_chain_tc at 1080p and 4K, in one process: HIP events around REPS back-to-back launches after a warm-up, the median of
    ROUNDS such measurements, alternating with the same arithmetic in torch ops on the device (elementwise passes and a bincount),
    next to the streaming floor: the bytes the launch must move -- 21 B per pixel read (flow x 2, cost, vis, sel, and the mask's
    byte), 16 B written (dst x 2, w, ok), 12 B without w; without the histogram the mask is not read -- over the HBM rate
    measured on this part by tools/bench_flow_chain.py (6.29 TB/s).  Every launch works on another of N buffer sets that
    together exceed the Infinity Cache.
(2) WOFTChained.track against MultiFlowTracker.track alone, per frame, for deltas (None,), (None, 1) and the default seven, on the
    synthetic checkpoint: host clock around FRAMES frames that end in a device synchronise, after a warm-up long enough for every
    delta to have a source frame, alternating rounds.  The difference is the planar stage: chain_tc, the selection, the fit and
    its one device -> host read, plus the histogram's read.
No GPU: the tool fails, it has no fallback."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.bench_flow_chain import CACHE_BYTES, HBM_MEASURED, K_REPS, K_ROUNDS, K_WARMUP, smooth_flow  # noqa: E402
from tools.bench_multiflow import DELTAS, FRAMES, ROUNDS, timed_pair  # noqa: E402
from tools.bench_window import SIZES  # noqa: E402

READ_BPP, MASK_BPP = 20, 1             # flow x 2, cost, vis, sel; the template mask's byte


def chain_tc_bytes(want_w):
    return READ_BPP + MASK_BPP + (16 if want_w else 12)


def chain_tc_by_torch_ops(flow, cost, vis, sel, tmask, thr, xs, ys, want_w, want_hist=True):
    """The arithmetic of woft_chain_tc in torch ops on the device -> (dst, w, ok, hist)."""
    valid = (sel >= 0) & (sel <= 127) & torch.isfinite(flow).all(0) & torch.isfinite(cost) & torch.isfinite(vis)
    nan = torch.full_like(cost, float("nan"))
    dst = torch.stack([torch.where(valid, xs + flow[0], nan), torch.where(valid, ys + flow[1], nan)])
    w = torch.where(valid, torch.exp(-cost), torch.zeros_like(cost)) if want_w else None
    seen = valid & ~(vis < thr)
    if not want_hist:
        return dst, w, seen.float(), None
    m = tmask != 0
    idx = torch.where(seen, sel, torch.where(valid, torch.full_like(sel, 129), torch.full_like(sel, 128)))
    hist = torch.bincount(idx[m].long(), minlength=130)
    return dst, w, seen.float(), hist


def bench_kernel(say):
    from woft_amd import ops
    say(f"# chain_tc: median over {K_ROUNDS} alternating measurements of {K_REPS} back-to-back calls (HIP events) after {K_WARMUP} "
        f"warm-up calls, rotating over buffer sets of >= {CACHE_BYTES >> 20} MiB in all; floor = bytes / {HBM_MEASURED / 1e12:.2f} TB/s")
    say("# size | form | woft_chain_tc ms (min-max) | torch ops ms (min-max) | floor ms (bytes per pixel) | chain_tc / floor | "
        "torch ops / chain_tc")
    for sname, (h, w) in SIZES.items():
        n = h * w
        n_sets = max(2, -(-CACHE_BYTES // (n * 37)))
        gen = lambda seed: torch.Generator(device="cuda").manual_seed(seed)
        plane = lambda lo, hi, seed: lo + (hi - lo) * torch.rand(h, w, device="cuda", generator=gen(seed))
        flow = [smooth_flow(h, w, 10 + i, 1.0) for i in range(n_sets)]
        cost, vis = [plane(0.0, 3.0, 50 + i) for i in range(n_sets)], [plane(0.2, 1.0, 90 + i) for i in range(n_sets)]
        # the winning candidate in blocks of 32 x 32 pixels, as a tracker's frames have it (a wave mostly agrees on it)
        sel = [torch.randint(0, 7, (h // 32 + 1, w // 32 + 1), device="cuda", generator=gen(130 + i), dtype=torch.int32)
               .repeat_interleave(32, 0).repeat_interleave(32, 1)[:h, :w].contiguous() for i in range(n_sets)]
        tmask = torch.zeros(h, w, dtype=torch.uint8, device="cuda")
        tmask[h // 4:3 * h // 4, w // 4:3 * w // 4] = 255
        ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32),
                                torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
        new = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        outs = [(new(2, n), new(1, n), new(1, n), torch.empty(130, dtype=torch.int32, device="cuda")) for _ in range(n_sets)]
        bare = [o[:3] + (None,) for o in outs]
        for name, want_w, sets in (("dst, w, ok, hist", True, outs), ("dst, ok, hist (no weights)", False, outs),
                                   ("dst, w, ok (no histogram: no counters, no zeroing launch)", True, bare)):
            want_hist = sets is outs
            k, t = timed_pair((lambda i: ops.chain_tc(flow[i], cost[i], vis[i], sel[i], tmask if want_hist else None, 0.5,
                                                      want_w=want_w, out=sets[i]),
                               lambda i: chain_tc_by_torch_ops(flow[i], cost[i], vis[i], sel[i], tmask, 0.5, xs, ys, want_w,
                                                               want_hist)), n_sets)
            bpp = chain_tc_bytes(want_w) - (0 if want_hist else MASK_BPP)
            floor = n * bpp / HBM_MEASURED * 1e3
            say(f"{sname} | {name} | {k[0]:.4f} ({k[1]:.4f}-{k[2]:.4f}) | {t[0]:.4f} ({t[1]:.4f}-{t[2]:.4f}) | {floor:.4f} ({bpp} B) | "
                f"x{k[0] / floor:.2f} | x{t[0] / k[0]:.1f}")
        del flow, cost, vis, sel, outs
        torch.cuda.empty_cache()


def bench_trackers(args, say):
    import bench
    from pytracking.utils.config import load_config
    from woft_amd import MultiFlowTracker, synth
    sd = synth.make_state_dict(seed=7)
    warm = max(d for d in DELTAS[-1] if d is not None) + 2
    say(f"# WOFTChained.track against MultiFlowTracker.track alone: {ROUNDS} alternating rounds x {FRAMES} frames per tracker after "
        f"{warm} warm-up frames each; raft_type 'weighted', {args.iters} flow iterations; host clock, one synchronise per round")
    say("# size | deltas | WOFTChained ms per frame (min-max of the rounds) | MultiFlowTracker ms per frame (min-max) | difference ms "
        "| difference / one flow (the deltas=(None,) MultiFlowTracker frame)")
    for sname in args.sizes:
        H, W = SIZES[sname]
        _, frames = bench.make_sequence(H, W, 0, bench.CLIP)
        mask = synth.make_init_mask(H, W)
        one_flow = None
        for deltas in DELTAS:
            conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained.py")
            conf.flow_config.model, conf.flow_config.iters, conf.chain_deltas = sd, args.iters, deltas
            planar = conf.tracker_class(conf)
            planar.init(frames[0], mask)
            fc = load_config(ROOT / "pytracking" / "optical_flow" / "configs" / "v2_SNOB_large_g05_RAFT.py")
            fc.model, fc.iters = sd, args.iters
            dense = MultiFlowTracker(fc.of_class(fc), deltas=deltas)
            dense.init(frames[0])
            step = {"planar": lambda: planar.track(frames[(planar.multi.frame_index + 1) % len(frames)]),
                    "dense": lambda: dense.track(frames[(dense.frame_index + 1) % len(frames)])}
            for fn in step.values():
                for _ in range(warm):
                    fn()
            torch.cuda.synchronize()
            ms = {name: [] for name in step}
            for r in range(ROUNDS):
                for name in (("planar", "dense") if r % 2 == 0 else ("dense", "planar")):
                    t0 = time.perf_counter()
                    for _ in range(FRAMES):
                        step[name]()
                    torch.cuda.synchronize()
                    ms[name].append((time.perf_counter() - t0) / FRAMES * 1e3)
            p, d = float(np.mean(ms["planar"])), float(np.mean(ms["dense"]))
            one_flow = d if one_flow is None else one_flow
            say(f"{sname} | {deltas!r} | {p:.2f} ({min(ms['planar']):.2f}-{max(ms['planar']):.2f}) | {d:.2f} "
                f"({min(ms['dense']):.2f}-{max(ms['dense']):.2f}) | {p - d:+.2f} | x{(p - d) / one_flow:.3f}")
            del planar, dense, step
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=["1080p"], choices=list(SIZES), help="frame sizes of the tracker part")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_chained.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/bench_chained.py on {torch.cuda.get_device_name(0)}")
    bench_kernel(say)
    bench_trackers(args, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
