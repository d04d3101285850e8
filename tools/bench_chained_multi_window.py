"""What the multi-target chained tracker on ONE union search window costs against the whole-frame multi-target tracker (DESIGN.md
section 28):

    python tools/bench_chained_multi_window.py --out profiles/chained_multi_window_bench.txt

(1) One woft_chain_tc_multi_window launch against K woft_chain_tc_window calls, and one woft_mask_bbox_multi launch against K
    woft_mask_bbox(mask_t, hinv_t) calls, K in 1, 4, 16: HIP events around back-to-back launches rotating over buffer sets that
    together exceed the Infinity Cache, next to the streaming floor -- the bytes counted from the arguments, over the HBM rate
    measured on this part by tools/bench_flow_chain.py (6.29 TB/s).
(2) WOFTChainedMultiWindow (pytracking/configs/WOFT_chained_multi_window.py, margin 0.25) against WOFTChainedMulti
    (WOFT_chained_multi.py) on identical frames, in one process: bench.py's sequences at 1080p and 4K, K in 1, 4, 16 masks of 1/16
    of each frame side, close together (one cluster at the centre) and spread out (one per cell of a grid over the frame), deltas
    (None, 1) and the default seven, the synthetic checkpoint.  Both trackers are warmed up long enough for every delta to have a
    source frame, then timed in alternating rounds (host clock around frames that end in a device synchronise); the spread of the
    rounds is printed next to the mean.  The yardstick is WOFTChainedMulti in the same process.
A combination left out by --ks / --sizes / --layouts / --deltas is written as "not measured".  No GPU: the tool fails, it has no
fallback."""
import argparse
import gc
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.bench_chained import READ_BPP  # noqa: E402
from tools.bench_chained_window import timed  # noqa: E402
from tools.bench_flow_chain import CACHE_BYTES, HBM_MEASURED, K_REPS, K_ROUNDS, K_WARMUP, smooth_flow  # noqa: E402
from tools.bench_window import SIZES  # noqa: E402

ROUNDS, FRAMES = 3, 8
KS = (1, 4, 16)
LAYOUTS = ("close", "spread")
DELTAS = {"(None, 1)": (None, 1), "default": (None, 1, 2, 4, 8, 16, 32)}
MASK_DIV = 16                                     # a mask's side = the frame's side / 16


def target_masks(H, W, K, layout):
    """K rectangular masks of (H / 16) x (W / 16) on a ceil(sqrt(K))-wide grid: 'close' with a pitch of 1.25 mask sides about the
    frame's centre, 'spread' with one mask in the middle of each cell of a grid over the whole frame."""
    h, w = H // MASK_DIV, W // MASK_DIV
    g = int(np.ceil(np.sqrt(K)))
    py, px = ((5 * h) // 4, (5 * w) // 4) if layout == "close" else (H // g, W // g)
    oy, ox = (H - py * g) // 2 + (py - h) // 2, (W - px * g) // 2 + (px - w) // 2
    masks = []
    for t in range(K):
        m = np.zeros((H, W), np.uint8)
        y0, x0 = oy + (t // g) * py, ox + (t % g) * px
        m[y0:y0 + h, x0:x0 + w] = 255
        masks.append(m)
    return masks


def chain_tc_multi_bytes(n, K):
    """Bytes one woft_chain_tc_multi_window launch must move, from its arguments: per pixel the five input planes and the bit
    plane's word read once, dst x 2, w and ok written; the K histograms zeroed and written."""
    return n * (READ_BPP + 4 + 16) + 2 * K * 130 * 4


def mask_bbox_multi_bytes(n, K):
    """... one woft_mask_bbox_multi launch: the bit plane read once (what a kernel that reads every word once would move; the
    launch gathers it K times through the caches), K rows of five ints written."""
    return 4 * n + 20 * K


def bench_kernels(args, say):
    from woft_amd import ops
    from woft_amd.chained import pack_target_bits
    from woft_amd.window import Box, chain_rect, union_box
    say(f"# kernels: median over {K_ROUNDS} measurements of {K_REPS} back-to-back launches (HIP events) after {K_WARMUP} warm-up "
        f"launches, rotating over buffer sets of >= {CACHE_BYTES >> 20} MiB in all; floor = bytes / {HBM_MEASURED / 1e12:.2f} TB/s; "
        "the window is the union window of the 'close' layout; 'K singles' is K calls of the single-target entry point")
    say("# size | K | launch | planes | ms per launch (min-max) | K singles ms | floor ms (bytes) | launch / floor | K singles / launch")
    for sname in args.sizes:
        H, W = SIZES[sname]
        for K in args.ks:
            masks = target_masks(H, W, K, "close")
            R0 = chain_rect(union_box([Box.from_mask(m) for m in masks]), 0.25, W, H)
            y0, x0, h, w = R0
            n = h * w
            n_sets = max(2, -(-CACHE_BYTES // (n * 60)))
            gen = lambda seed: torch.Generator(device="cuda").manual_seed(seed)
            plane = lambda lo, hi, seed: lo + (hi - lo) * torch.rand(h, w, device="cuda", generator=gen(seed))
            folds = [(smooth_flow(h, w, 10 + i, 1.0), plane(0.0, 3.0, 50 + i), plane(0.2, 1.0, 90 + i),
                      torch.randint(0, 7, (h, w), device="cuda", dtype=torch.int32, generator=gen(130 + i))) for i in range(n_sets)]
            bits = pack_target_bits(masks)
            tb_full = torch.from_numpy(bits.view(np.int32)).cuda()
            tb = torch.from_numpy(np.ascontiguousarray(bits[y0:y0 + h, x0:x0 + w]).view(np.int32)).cuda()
            crops = [torch.from_numpy(np.ascontiguousarray(m[y0:y0 + h, x0:x0 + w])).cuda() for m in masks]
            new = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
            outs = [(new(2, n), new(1, n), new(1, n), torch.empty(K, 130, dtype=torch.int32, device="cuda")) for _ in range(n_sets)]
            outs1 = [(o[0], o[1], o[2], o[3][0]) for o in outs]
            t = timed(lambda i: ops.chain_tc_multi_window(*folds[i], tb, K, 0.5, (y0, x0), (H, W), out=outs[i]), n_sets)
            s = timed(lambda i: [ops.chain_tc_window(*folds[i], crops[k], 0.5, (y0, x0), (H, W), out=outs1[i]) for k in range(K)], n_sets)
            nbytes = chain_tc_multi_bytes(n, K)
            floor = nbytes / HBM_MEASURED * 1e3
            say(f"{sname} | {K} | chain_tc_multi_window | {h} x {w} window | {t[0]:.4f} ({t[1]:.4f}-{t[2]:.4f}) | {s[0]:.4f} | "
                f"{floor:.4f} ({nbytes / 1e6:.1f} MB) | x{t[0] / floor:.2f} | x{s[0] / t[0]:.2f}")
            del folds, outs, outs1, crops, tb
            # the boxes of the K masks, each carried by a pose of its own (a small rotation, scale and shift)
            poses = []
            for k in range(K):
                a = 0.01 * (k + 1)
                poses.append(np.array([[1.01 * np.cos(a), -np.sin(a), 5.0 + k], [np.sin(a), 0.99 * np.cos(a), -3.0 + k], [1e-6, 0, 1.0]]))
            full = [torch.from_numpy(m).cuda() for m in masks]
            rows = torch.empty(K, 5, dtype=torch.int32, device="cuda")
            row1 = torch.empty(5, dtype=torch.int32, device="cuda")
            t = timed(lambda i: ops.mask_bbox_multi(tb_full, K, poses, bbox=rows), 1)
            s = timed(lambda i: [ops.mask_bbox(full[k], bbox=row1, Hmat=poses[k]) for k in range(K)], 1)
            nbytes = mask_bbox_multi_bytes(H * W, K)
            floor = nbytes / HBM_MEASURED * 1e3
            say(f"{sname} | {K} | mask_bbox_multi | {H} x {W} frame | {t[0]:.4f} ({t[1]:.4f}-{t[2]:.4f}) | {s[0]:.4f} | "
                f"{floor:.4f} ({nbytes / 1e6:.1f} MB) | x{t[0] / floor:.2f} | x{s[0] / t[0]:.2f}")
            del full, tb_full
            torch.cuda.empty_cache()


def make_tracker(cfg, sd, iters, deltas, frame0, masks):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / cfg)
    conf.flow_config.model, conf.flow_config.iters, conf.chain_deltas = sd, iters, deltas
    conf.flow_config.padding_mode = "RAFT"           # (both trackers: a whole side of a window need be no multiple of 8)
    trk = conf.tracker_class(conf)
    trk.init(frame0, masks)
    return trk


def bench_trackers(args, say):
    import bench
    from woft_amd import synth
    sd = synth.make_state_dict(seed=7)
    say(f"# WOFTChainedMultiWindow against WOFTChainedMulti: {args.rounds} alternating rounds x {args.frames} frames per tracker after a "
        f"warm-up of (largest delta + 2) frames each; raft_type 'weighted', {args.iters} flow iterations; masks of 1/{MASK_DIV} of each "
        "frame side; host clock, one synchronise per round.  A flow is about 200 launches whatever its size: that floor bounds the gain.")
    say("# size K layout | deltas | WOFTChainedMulti ms per frame (min-max of the rounds) | WOFTChainedMultiWindow ms per frame (min-max) | "
        "template rect R0 | windows of the timed frames (distinct rects) | plans kept | whole-frame / window")
    for sname in SIZES:
        H, W = SIZES[sname]
        frames = None
        for K in KS:
            for layout in LAYOUTS:
                for dname, deltas in DELTAS.items():
                    if sname not in args.sizes or K not in args.ks or layout not in args.layouts or dname not in args.deltas:
                        say(f"{sname} K={K} {layout} | {dname} | not measured")
                        continue
                    if frames is None:
                        _, frames = bench.make_sequence(H, W, 0, bench.CLIP)
                    masks = target_masks(H, W, K, layout)
                    trk = {"full": make_tracker("WOFT_chained_multi.py", sd, args.iters, deltas, frames[0], masks),
                           "win": make_tracker("WOFT_chained_multi_window.py", sd, args.iters, deltas, frames[0], masks)}
                    rects = set()

                    def step(name):
                        t = trk[name]
                        _, metas = t.track(frames[(t.multi.frame_index + 1) % len(frames)])
                        if name == "win":
                            rects.add(metas[0].chain_window)
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
                    say(f"{sname} K={K} {layout} | {dname} | {f:.2f} ({min(ms['full']):.2f}-{max(ms['full']):.2f}) | {w:.2f} "
                        f"({min(ms['win']):.2f}-{max(ms['win']):.2f}) | {R0[2]} x {R0[3]} at ({R0[0]}, {R0[1]}) of {H} x {W} | "
                        f"{len(rects)}: {sorted({r[2:] for r in rects})} | {len(trk['win'].flower.engine._plans)} | x{f / w:.2f}")
                    del trk, step
                    gc.collect()                           # (a tracker and its provider's plans sit in reference cycles)
                    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--ks", nargs="+", type=int, default=list(KS), choices=list(KS))
    ap.add_argument("--layouts", nargs="+", default=list(LAYOUTS), choices=list(LAYOUTS))
    ap.add_argument("--deltas", nargs="+", default=list(DELTAS), choices=list(DELTAS))
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--no-trackers", action="store_true", help="the kernel part only; every tracker row reads 'not measured'")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_chained_multi_window.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                   # (rewritten line by line: a run that is cut short leaves what it measured)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")
    say(f"# tools/bench_chained_multi_window.py on {torch.cuda.get_device_name(0)}")
    bench_kernels(args, say)
    if args.no_trackers:
        args.sizes = []
    bench_trackers(args, say)


if __name__ == "__main__":
    main()
