"""What the chained tracker on search windows costs against the whole-frame chained tracker:

    python tools/bench_chained_window.py --out profiles/chained_window_bench.txt

(1) WOFTChainedWindow (pytracking/configs/WOFT_chained_window.py, margin 0.25) against WOFTChained (WOFT_chained.py) on identical
    frames, in one process: bench.py's sequences at 1080p and 4K, centred masks covering 1/4, 1/16 and 1/64 of the frame, deltas
    (None, 1) and the default seven, the synthetic checkpoint.  Both trackers are warmed up long enough for every delta to have a
    source frame, then timed in alternating rounds (host clock around frames that end in a device synchronise); the spread of the
    rounds is printed next to the mean.  The yardstick is WOFTChained in the same process.  A flow is about 200 launches whatever
    its size: that floor bounds the gain of a window, as it does for WOFTWindow.
(2) One woft_flow_chain_fold_window and one woft_chain_tc_window launch on the 1/4 mask's window of each size: HIP events around
    back-to-back launches rotating over buffer sets that together exceed the Infinity Cache, next to the streaming floor -- the
    bytes counted from the arguments, over the HBM rate measured on this part by tools/bench_flow_chain.py (6.29 TB/s).
No GPU: the tool fails, it has no fallback."""
import argparse
import gc
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.bench_chained import chain_tc_bytes  # noqa: E402
from tools.bench_flow_chain import CACHE_BYTES, HBM_MEASURED, K_REPS, K_ROUNDS, K_WARMUP, smooth_flow  # noqa: E402
from tools.bench_window import MASKS, SIZES, centred_mask  # noqa: E402

ROUNDS, FRAMES = 3, 8
DELTAS = ((None, 1), (None, 1, 2, 4, 8, 16, 32))


def fold_window_bytes(n_t, n_s, prev, wlogit, mlogit, first, replaced):
    """Bytes one fold launch on rectangles must move, from its arguments (tools/bench_multiflow.fold_bytes with two pixel counts):
    over the n_t template-rectangle pixels the prev planes (flow x 2, cost, vis) read once, of the running best sel, cost and vis
    read unless `first` and all five planes written where the candidate replaces it (`replaced`: that share, 1 with `first`);
    over the n_s step-rectangle pixels the step planes (flow x 2 and each logit given) read once."""
    per_t = (4 if prev else 0) + (0 if first else 3) + 5 * (1.0 if first else replaced)
    return 4 * (per_t * n_t + (2 + bool(wlogit) + bool(mlogit)) * n_s)


def make_tracker(cfg, sd, iters, deltas, frame0, mask):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / cfg)
    conf.flow_config.model, conf.flow_config.iters, conf.chain_deltas = sd, iters, deltas
    conf.flow_config.padding_mode = "RAFT"           # (both trackers: a whole side of a window need be no multiple of 8)
    trk = conf.tracker_class(conf)
    trk.init(frame0, mask)
    return trk


def bench_trackers(args, say):
    import bench
    from woft_amd import synth
    sd = synth.make_state_dict(seed=7)
    say(f"# WOFTChainedWindow against WOFTChained: {args.rounds} alternating rounds x {args.frames} frames per tracker after a warm-up "
        f"of (largest delta + 2) frames each; raft_type 'weighted', {args.iters} flow iterations; host clock, one synchronise per "
        "round.  A flow is about 200 launches whatever its size: that floor bounds the gain.")
    say("# size mask | deltas | WOFTChained ms per frame (min-max of the rounds) | WOFTChainedWindow ms per frame (min-max) | "
        "template rect R0 | windows of the timed frames (distinct rects) | plans kept | whole-frame / window")
    for sname in args.sizes:
        H, W = SIZES[sname]
        _, frames = bench.make_sequence(H, W, 0, bench.CLIP)
        for mname, k in MASKS.items():
            mask = centred_mask(H, W, k)
            for deltas in DELTAS:
                trk = {"full": make_tracker("WOFT_chained.py", sd, args.iters, deltas, frames[0], mask),
                       "win": make_tracker("WOFT_chained_window.py", sd, args.iters, deltas, frames[0], mask)}
                rects = set()

                def step(name):
                    t = trk[name]
                    _, meta = t.track(frames[(t.multi.frame_index + 1) % len(frames)])
                    if name == "win":
                        rects.add(meta.chain_window)
                warm = max(d for d in deltas if d is not None) + 2
                for name in trk:
                    for _ in range(warm):
                        step(name)
                torch.cuda.synchronize()
                rects.clear()
                ms = {name: [] for name in trk}
                for r in range(args.rounds):
                    for name in (("full", "win") if r % 2 == 0 else ("win", "full")):
                        t0 = time.perf_counter()
                        for _ in range(args.frames):
                            step(name)
                        torch.cuda.synchronize()
                        ms[name].append((time.perf_counter() - t0) / args.frames * 1e3)
                f, w = float(np.mean(ms["full"])), float(np.mean(ms["win"]))
                R0 = trk["win"].multi.rect0
                say(f"{sname} {mname} | {deltas!r} | {f:.2f} ({min(ms['full']):.2f}-{max(ms['full']):.2f}) | {w:.2f} "
                    f"({min(ms['win']):.2f}-{max(ms['win']):.2f}) | {R0[2]} x {R0[3]} at ({R0[0]}, {R0[1]}) of {H} x {W} | "
                    f"{len(rects)}: {sorted({r[2:] for r in rects})} | {len(trk['win'].flower.engine._plans)} | x{f / w:.2f}")
                del trk, step
                gc.collect()                           # (a tracker and its provider's plans sit in reference cycles)
                torch.cuda.empty_cache()


def timed(fn, n_sets):
    """Median (min, max) ms per call."""
    for i in range(K_WARMUP):
        fn(i % n_sets)
    torch.cuda.synchronize()
    ms = []
    for _ in range(K_ROUNDS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(K_REPS):
            fn(i % n_sets)
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e) / K_REPS)
    return float(np.median(ms)), min(ms), max(ms)


def bench_kernels(say):
    from woft_amd import ops
    from woft_amd.window import Box, chain_rect
    say(f"# kernels: median over {K_ROUNDS} measurements of {K_REPS} back-to-back launches (HIP events) after {K_WARMUP} warm-up "
        f"launches, rotating over buffer sets of >= {CACHE_BYTES >> 20} MiB in all; floor = bytes / {HBM_MEASURED / 1e12:.2f} TB/s; "
        "template rect = step rect shifted by (8, 8): the 1/4 mask's window")
    say("# size | window | launch | ms per launch (min-max) | floor ms (bytes) | launch / floor")
    for sname, (H, W) in SIZES.items():
        R0 = chain_rect(Box.from_mask(centred_mask(H, W, 2)), 0.25, W, H)
        y0, x0, h, w = R0
        S = (max(y0 - 8, 0), max(x0 - 8, 0), h, w)
        n = h * w
        n_sets = max(2, -(-CACHE_BYTES // (n * 64)))
        gen = lambda seed: torch.Generator(device="cuda").manual_seed(seed)
        plane = lambda lo, hi, seed: lo + (hi - lo) * torch.rand(h, w, device="cuda", generator=gen(seed))
        prev = [(smooth_flow(h, w, 10 + i, 1.0), plane(0.0, 3.0, 50 + i), plane(0.2, 1.0, 90 + i)) for i in range(n_sets)]
        step = [(smooth_flow(h, w, 130 + i, -1.0), plane(2.0, 4.0, 170 + i), plane(2.0, 4.0, 210 + i)) for i in range(n_sets)]
        best = [ops.flow_chain_fold_window(None, prev[(i + 1) % n_sets], *step[(i + 1) % n_sets], k=0, template_rect=R0, step_rect=S,
                                           first=True) for i in range(n_sets)]
        keep = [tuple(b.clone() for b in bb) for bb in best]
        Hm = np.array([[1.0, 0.002, -3.0], [-0.001, 1.0, 2.0], [1e-6, 0.0, 1.0]])
        # the share a later fold replaces, measured once on a copy
        trial = ops.flow_chain_fold_window(tuple(b.clone() for b in keep[0]), prev[0], *step[0], k=1, template_rect=R0, step_rect=S)
        replaced = float((trial[3] == 1).float().mean())
        forms = (("first fold, prev + both logits", dict(first=True), fold_window_bytes(n, n, True, True, True, True, 1.0)),
                 ("first fold, no prev, post_H (fp64)", dict(first=True, post_H=Hm, no_prev=True),
                  fold_window_bytes(n, n, False, True, True, True, 1.0)),
                 (f"later fold, prev + both logits, {replaced:.2f} replaced", dict(first=False),
                  fold_window_bytes(n, n, True, True, True, False, replaced)))
        for name, kw, nbytes in forms:
            no_prev = kw.pop("no_prev", False)

            def fold(i):
                if not kw["first"]:                    # (restore the running best: every launch replaces the same share)
                    for b, c in zip(best[i], keep[i]):
                        b.copy_(c)
                ops.flow_chain_fold_window(best[i], None if no_prev else prev[i], *step[i], k=1, template_rect=R0, step_rect=S, **kw)
            restore = 0.0
            if not kw["first"]:
                restore = timed(lambda i: [b.copy_(c) for b, c in zip(best[i], keep[i])], n_sets)[0]
            t = timed(fold, n_sets)
            floor = nbytes / HBM_MEASURED * 1e3
            say(f"{sname} | {h} x {w} | fold_window: {name} | {t[0] - restore:.4f} ({t[1] - restore:.4f}-{t[2] - restore:.4f}) | "
                f"{floor:.4f} ({nbytes / 1e6:.1f} MB) | x{(t[0] - restore) / floor:.2f}"
                + (f" (the {restore:.4f} ms of restoring the running best taken off)" if restore else ""))
        tmask = torch.full((h, w), 255, dtype=torch.uint8, device="cuda")
        new = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        outs = [(new(2, n), new(1, n), new(1, n), torch.empty(130, dtype=torch.int32, device="cuda")) for _ in range(n_sets)]
        t = timed(lambda i: ops.chain_tc_window(keep[i][0], keep[i][1], keep[i][2], keep[i][3], tmask, 0.5, (y0, x0), (H, W),
                                                out=outs[i]), n_sets)
        nbytes = n * chain_tc_bytes(True)
        floor = nbytes / HBM_MEASURED * 1e3
        say(f"{sname} | {h} x {w} | chain_tc_window: dst, w, ok, hist | {t[0]:.4f} ({t[1]:.4f}-{t[2]:.4f}) | {floor:.4f} "
            f"({nbytes / 1e6:.1f} MB) | x{t[0] / floor:.2f}")
        del prev, step, best, keep, outs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES), help="frame sizes of the tracker part")
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_chained_window.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/bench_chained_window.py on {torch.cuda.get_device_name(0)}")
    bench_kernels(say)
    bench_trackers(args, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
