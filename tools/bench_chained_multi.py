"""What tracking K planar targets on one chained flow costs:

    python tools/bench_chained_multi.py --out profiles/chained_multi_bench.txt

(1) woft_chain_tc_multi at 1080p and 4K for K in {1, 4, 16, 32}: HIP events around REPS back-to-back launches after a warm-up, the
    median of ROUNDS such measurements, next to the streaming floor -- 40 B per pixel with weights: flow 8, cost, vis, sel and the
    bit plane 4 each read, dst 8, w and ok 4 each written -- over the HBM rate measured on this part by tools/bench_flow_chain.py
    (6.29 TB/s).  Every launch works on another of N buffer sets that together exceed the Infinity Cache.
(2) The planar stage of K targets on one fold result, batched (chain_tc_multi, tc_select_multi, hfit_batched, inlier_frac_batched,
    one pinned read) against a loop of K single-target stages through the entry points the tree had before (chain_tc,
    tc_select_vis, hfit, inlier_frac, the pinned read and the histogram's read: what K WOFTChained trackers run after their dense
    track), in one process, alternating rounds, on the same fold result: device time (HIP events around REPS enqueue-only
    repetitions, no read-back) and wall time per stage including its read-backs (host clock).
(3) WOFTChainedMulti.track against K WOFTChained.track for K = 4 with deltas (None, 1) on the synthetic checkpoint, per frame:
    host clock around FRAMES frames that end in a device synchronise, alternating rounds.
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
from tools.bench_multiflow import FRAMES, ROUNDS, timed_pair  # noqa: E402
from tools.bench_window import SIZES  # noqa: E402

KS = (1, 4, 16, 32)
MULTI_BPP = 40                         # flow 8, cost, vis, sel, tbits 4 each; dst 8, w, ok 4 each
N_DRAW, CAP, THR = 500, 1024, 5.0


def target_masks(h, w, K):
    """K overlapping rectangles of a quarter of the frame's sides, spread along its diagonal -> (K, h, w) uint8 numpy."""
    m = np.zeros((K, h, w), np.uint8)
    for t in range(K):
        y0, x0 = (h - h // 4) * t // max(K, 2), (w - w // 4) * t // max(K, 2)
        m[t, y0:y0 + h // 4, x0:x0 + w // 4] = 255
    return m


def fold_result(h, w, seed):
    """A fold result as a tracker's frames have it: a smooth flow, costs, mostly visible, the winning candidate in 32 x 32 blocks."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    plane = lambda lo, hi: lo + (hi - lo) * torch.rand(h, w, device="cuda", generator=gen)
    sel = (torch.randint(0, 7, (h // 32 + 1, w // 32 + 1), device="cuda", generator=gen, dtype=torch.int32)
           .repeat_interleave(32, 0).repeat_interleave(32, 1)[:h, :w].contiguous())
    return smooth_flow(h, w, seed, 1.0), plane(0.0, 3.0), plane(0.2, 1.0), sel


class Stage:
    """The buffers and the two forms of the planar stage of K targets at one size."""

    def __init__(self, h, w, K):
        from woft_amd import ops, presets
        from woft_amd.chained import pack_target_bits
        self.ops, self.h, self.w, self.K = ops, h, w, K
        n = h * w
        masks = target_masks(h, w, K)
        self.tbits = torch.from_numpy(pack_target_bits(list(masks)).view(np.int32)).cuda()
        self.masks = [torch.from_numpy(m).cuda() for m in masks]
        self.sobol = torch.from_numpy(presets.sobol_points(N_DRAW).astype(np.float32)).cuda()
        new = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        # batched
        self.blk = torch.zeros(K * (13 + ops.CHAIN_HIST), dtype=torch.float32, device="cuda")
        ib = self.blk.view(torch.int32)
        self.H, self.frac, self.status = self.blk[:9 * K].view(K, 9), self.blk[9 * K:10 * K], ib[10 * K:11 * K]
        self.count, self.hist = ib[11 * K:13 * K].view(2, K), ib[13 * K:].view(K, ops.CHAIN_HIST)
        self.tc = (new(2, n), new(1, n), new(1, n), self.hist)
        self.ws, self.pa, self.pb, self.wo = ops.tc_select_multi_ws(n, K), new(K, CAP, 2), new(K, CAP, 2), new(K, CAP)
        self.host = torch.empty(self.blk.numel(), dtype=torch.float32).pin_memory()
        # the loop's single-target buffers (one set, reused target after target, as K trackers of one process would not -- theirs
        # are K sets; the launches and reads are the same)
        self.tc1 = (new(2, n), new(1, n), new(1, n), torch.empty(ops.CHAIN_HIST, dtype=torch.int32, device="cuda"))
        self.ws1, self.pa1, self.pb1, self.wo1 = ops.tc_select_ws(n), new(CAP, 2), new(CAP, 2), new(CAP)
        self.res = torch.zeros(16, dtype=torch.float32, device="cuda")
        self.host1 = torch.empty(16, dtype=torch.float32).pin_memory()
        self.event = torch.cuda.Event()

    def batched(self, fold, read):
        ops, K = self.ops, self.K
        flow, cost, vis, sel = fold
        dst, w, ok, _ = ops.chain_tc_multi(flow, cost, vis, sel, self.tbits, K, 0.5, out=self.tc)
        ops.tc_select_multi(dst, w, self.tbits, K, self.h, self.w, True, self.sobol, ok, "gate", 0.5, self.ws, self.pa, self.pb,
                            self.wo, self.count)
        ops.hfit_batched(self.pa, self.pb, self.wo, self.H, self.status, counts=self.count[0])
        ops.inlier_frac_batched(self.pa, self.pb, self.H, self.frac, thr=THR, counts=self.count[0])
        if read:
            self.host.copy_(self.blk, non_blocking=True)
            self.event.record()
            self.event.synchronize()

    def loop(self, fold, read):
        ops = self.ops
        flow, cost, vis, sel = fold
        ires = self.res.view(torch.int32)
        for t in range(self.K):
            dst, w, ok, hist = ops.chain_tc(flow, cost, vis, sel, self.masks[t], 0.5, out=self.tc1)
            ops.tc_select_vis(dst, w, self.masks[t], None, self.h, self.w, True, self.sobol, ok, "gate", 0.5, self.ws1, self.pa1,
                              self.pb1, self.wo1, ires[12:14])
            ops.hfit(self.pa1, self.pb1, self.wo1, self.res[0:9], ires[10:11], count=ires[12:13])
            ops.inlier_frac(self.pa1, self.pb1, self.res[0:9], self.res[9:10], thr=THR, count=ires[12:13])
            if read:
                self.host1.copy_(self.res, non_blocking=True)
                self.event.record()
                self.event.synchronize()
                hist.cpu()


def wall_pair(fns, n_sets):
    """Median (min, max) ms per call of each function by the host clock, the device idle before and after; alternating rounds."""
    ms = [[] for _ in fns]
    for fn in fns:
        for i in range(4):
            fn(i % n_sets)
    for _ in range(K_ROUNDS):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(K_REPS):
                fn(i % n_sets)
            torch.cuda.synchronize()
            ms[j].append((time.perf_counter() - t0) / K_REPS * 1e3)
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def bench_stage(say):
    from woft_amd import ops
    say(f"# median over {K_ROUNDS} alternating measurements of {K_REPS} back-to-back repetitions after {K_WARMUP} warm-up ones, rotating "
        f"over fold results of >= {CACHE_BYTES >> 20} MiB in all; floor = {MULTI_BPP} B per pixel / {HBM_MEASURED / 1e12:.2f} TB/s; "
        f"Sobol draw {N_DRAW}, weighted least squares; masks: K overlapping rectangles of a quarter of the frame's sides")
    say("# size | K | chain_tc_multi ms (min-max) | floor ms | chain_tc_multi / floor | device ms: batched stage (min-max) | loop of K "
        "single stages (min-max) | loop / batched | wall ms with read-backs: batched (min-max) | loop (min-max) | loop / batched")
    fmt = lambda v: f"{v[0]:.4f} ({v[1]:.4f}-{v[2]:.4f})"
    for sname, (h, w) in SIZES.items():
        n = h * w
        n_sets = max(2, -(-CACHE_BYTES // (n * MULTI_BPP)))
        folds = [fold_result(h, w, 10 + i) for i in range(n_sets)]
        floor = n * MULTI_BPP / HBM_MEASURED * 1e3
        for K in KS:
            S = Stage(h, w, K)
            one = lambda i: ops.chain_tc_multi(*folds[i], S.tbits, K, 0.5, out=S.tc)
            k, _ = timed_pair((one, one), n_sets)
            dev_b, dev_l = timed_pair((lambda i: S.batched(folds[i], False), lambda i: S.loop(folds[i], False)), n_sets)
            wall_b, wall_l = wall_pair((lambda i: S.batched(folds[i], True), lambda i: S.loop(folds[i], True)), n_sets)
            say(f"{sname} | {K} | {fmt(k)} | {floor:.4f} | x{k[0] / floor:.2f} | {fmt(dev_b)} | {fmt(dev_l)} | x{dev_l[0] / dev_b[0]:.1f} | "
                f"{fmt(wall_b)} | {fmt(wall_l)} | x{wall_l[0] / wall_b[0]:.1f}")
            del S
        del folds
        torch.cuda.empty_cache()


def bench_trackers(args, say):
    import bench
    from pytracking.utils.config import load_config
    from woft_amd import synth
    K, deltas = 4, (None, 1)
    sd = synth.make_state_dict(seed=7)
    say(f"# WOFTChainedMulti.track (K = {K}) against {K} WOFTChained.track, deltas {deltas}: {ROUNDS} alternating rounds x {FRAMES} frames "
        f"after 3 warm-up frames; raft_type 'weighted', {args.iters} flow iterations; host clock, one synchronise per round")
    say(f"# size | WOFTChainedMulti ms per frame (min-max of the rounds) | {K} x WOFTChained ms per frame (min-max) | ratio")
    for sname in args.sizes:
        H, W = SIZES[sname]
        _, frames = bench.make_sequence(H, W, 0, bench.CLIP)
        masks = list(target_masks(H, W, K))

        def make(name):
            conf = load_config(ROOT / "pytracking" / "configs" / name)
            conf.flow_config.model, conf.flow_config.iters, conf.chain_deltas = sd, args.iters, deltas
            return conf.tracker_class(conf)
        multi = make("WOFT_chained_multi.py")
        multi.init(frames[0], masks)
        singles = [make("WOFT_chained.py") for _ in range(K)]
        for trk, m in zip(singles, masks):
            trk.init(frames[0], m)
        nxt = lambda trk: frames[(trk.multi.frame_index + 1) % len(frames)]
        step = {"multi": lambda: multi.track(nxt(multi)), "singles": lambda: [trk.track(nxt(trk)) for trk in singles]}
        for fn in step.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in step}
        for r in range(ROUNDS):
            for name in (("multi", "singles") if r % 2 == 0 else ("singles", "multi")):
                t0 = time.perf_counter()
                for _ in range(FRAMES):
                    step[name]()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / FRAMES * 1e3)
        a, b = float(np.mean(ms["multi"])), float(np.mean(ms["singles"]))
        say(f"{sname} | {a:.2f} ({min(ms['multi']):.2f}-{max(ms['multi']):.2f}) | {b:.2f} ({min(ms['singles']):.2f}-"
            f"{max(ms['singles']):.2f}) | x{b / a:.2f}")
        del multi, singles, step
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=["1080p"], choices=list(SIZES), help="frame sizes of the tracker part")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_chained_multi.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/bench_chained_multi.py on {torch.cuda.get_device_name(0)}")
    bench_stage(say)
    bench_trackers(args, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
