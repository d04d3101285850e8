"""What frame-features records cost and what they save:

    python tools/bench_features.py --out profiles/feature_share_bench.txt

One process; every comparison in alternating rounds; HIP events around back-to-back calls after a warm-up (the tracker rows: host
clock around frames that end in a device synchronise, as tools/bench_multiflow.py).
(1) woft_features_pack and woft_features_unpack in both roles at 1080p and 4K on the full model's channel counts, next to the
    streaming floor: the bytes the launch must move, counted from its arguments by `launch_bytes`, over the HBM rate measured on
    this part by tools/bench_flow_chain.py (6.29 TB/s).  Every launch works on another of N buffer sets that together exceed
    twice the 256 MiB Infinity Cache.
(2) provider.encode_frame (upload excluded: the frame is a device tensor).
(3) One chained flow -- a flow between two frames that are not the pinned template, as MultiFlowTracker runs them, in the second
    buffer set -- from the two images against the same flow from their two records.
(4) MultiFlowTracker.track at 1080p for deltas (None,), (None, 1) and the default seven, share_features off and on.
(5) compute_flow_fb, share_features off and on.
Synthetic checkpoint, raft_type 'weighted', the shipped arithmetic (bf16x3, corr 'otf').  No GPU: the tool fails, it has no
fallback."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.bench_flow_chain import CACHE_BYTES, HBM_MEASURED, K_REPS, K_ROUNDS, K_WARMUP  # noqa: E402
from tools.bench_multiflow import DELTAS  # noqa: E402
from tools.bench_window import SIZES  # noqa: E402

ROUNDS, FRAMES = 3, 12
F_REPS, F_ROUNDS, F_WARMUP = 6, 5, 3              # whole flows and encoder passes: milliseconds each
DIMS = (256, 128, 128)                            # fdim, hdim, cdim of the full model
XCS = 256                                         # channel stride of its GRU input buffer [inp | motion | flow | pad]


def launch_bytes(P, role):
    """Bytes one launch must move, from its arguments: every map read once and written once, fp32; the source role also writes
    inp a second time (inp_c) and the [hi | lo] bf16 lines of the fnet map (2 x 2 bytes per value)."""
    fdim, hdim, cdim = DIMS
    if role == "target":
        return 4 * P * fdim * 2
    read = 4 * P * (fdim + hdim + cdim)
    if role == "pack":
        return 2 * read
    return read + 4 * P * (fdim + hdim + 2 * cdim) + 2 * 2 * P * fdim


def timed(fns, n_sets, reps, rounds, warmup):
    """Median (min, max) ms per call of each function, measured in alternating rounds."""
    for fn in fns:
        for i in range(warmup):
            fn(i % n_sets)
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for j, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(reps):
                fn(i % n_sets)
            e.record()
            e.synchronize()
            ms[j].append(s.elapsed_time(e) / reps)
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def padded_pixels(sname):
    h, w = SIZES[sname]
    return ((h + 7) // 8) * ((w + 7) // 8)


def bench_kernels(args, say):
    from woft_amd import ops
    fdim, hdim, cdim = DIMS
    say(f"# launches: median over {K_ROUNDS} alternating measurements of {K_REPS} back-to-back calls (HIP events) after {K_WARMUP} "
        f"warm-up calls, rotating over buffer sets of >= {CACHE_BYTES >> 20} MiB in all; full model (fdim, hdim, cdim) = {DIMS}, "
        f"GRU input rows of {XCS} floats; floor = bytes / {HBM_MEASURED / 1e12:.2f} TB/s")
    say("# size (P) | launch | us (min-max) | MB moved | floor us | launch / floor | record MB")
    for sname in args.sizes:
        P = padded_pixels(sname)
        rows = (P + 127) // 128 * 128
        rec_floats = ops.features_record_floats(P, *DIMS)
        per_set = 4 * rec_floats + 4 * rows * fdim * 2 + 2 * rows * 2 * fdim + 4 * P * (hdim + XCS + cdim)
        n_sets = max(2, -(-CACHE_BYTES // per_set))
        g = torch.Generator(device="cuda").manual_seed(1)
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda")
        sets = []
        for _ in range(n_sets):
            f1rows = z(rows, fdim)
            f1rows[:P] = torch.randn(P, fdim, device="cuda", generator=g)
            sets.append(dict(rec=z(rec_floats), f1rows=f1rows, f1s=z(rows, 2 * fdim, dtype=torch.bfloat16),
                             net=torch.randn(P, hdim, device="cuda", generator=g), xbuf=torch.randn(P, XCS, device="cuda", generator=g),
                             inp_c=z(P, cdim), f2=z(P, fdim)))
        pack = lambda i: ops.features_pack(sets[i]["f1rows"], sets[i]["net"], sets[i]["xbuf"], P, DIMS, sets[i]["rec"])
        src = lambda i: ops.features_unpack(sets[i]["rec"], P, DIMS, sets[i]["f1rows"], sets[i]["f1s"], sets[i]["net"], sets[i]["xbuf"],
                                            sets[i]["inp_c"])
        dst = lambda i: ops.features_unpack(sets[i]["rec"], P, DIMS, sets[i]["f2"])
        res = timed((pack, src, dst), n_sets, K_REPS, K_ROUNDS, K_WARMUP)
        for (name, role), r in zip((("woft_features_pack", "pack"), ("woft_features_unpack, source role + split", "source"),
                                    ("woft_features_unpack, target role", "target")), res):
            nbytes = launch_bytes(P, role)
            floor = nbytes / HBM_MEASURED * 1e6
            say(f"{sname} ({P}) | {name} | {r[0] * 1e3:.1f} ({r[1] * 1e3:.1f}-{r[2] * 1e3:.1f}) | {nbytes / 1e6:.1f} | {floor:.1f} | "
                f"x{r[0] * 1e3 / floor:.2f} | {4 * rec_floats / 1e6:.1f}")
        del sets
        torch.cuda.empty_cache()


def _provider(args):
    from pytracking.utils.config import load_config
    from woft_amd import synth
    fc = load_config(ROOT / "pytracking" / "optical_flow" / "configs" / "v2_SNOB_large_g05_RAFT.py")
    fc.model, fc.iters = synth.make_state_dict(seed=7), args.iters
    return fc.of_class(fc)


def bench_flows(args, say):
    import bench
    say(f"# encode_frame, one chained flow and compute_flow_fb: median over {F_ROUNDS} alternating measurements of {F_REPS} back-to-back "
        f"calls (HIP events) after {F_WARMUP} warm-up calls; raft_type 'weighted', {args.iters} flow iterations; frames are device "
        "tensors; the chained flow runs beside a pinned template, mode 'flow', borrow=True")
    say("# size | what | ms (min-max) | against the row above")
    for sname in args.sizes:
        H, W = SIZES[sname]
        _, frames = bench.make_sequence(H, W, 0, 4)
        prov = _provider(args)
        prov.pin_source(frames[0])
        prov.compute_flow(frames[0], frames[1], mode="flow", borrow=True)
        a, b = frames[1], frames[2]
        ra, rb = prov.encode_frame(a), prov.encode_frame(b)
        enc = lambda i: prov.encode_frame(a)
        from_images = lambda i: prov.compute_flow(a, b, mode="flow", do_sigmoid=False, borrow=True)
        from_records = lambda i: prov.compute_flow(ra, rb, mode="flow", do_sigmoid=False, borrow=True)
        fb_off = lambda i: prov.compute_flow_fb(a, b)
        fb_on = lambda i: prov.compute_flow_fb(a, b, share_features=True)
        e, fi, fr, f0, f1 = timed((enc, from_images, from_records, fb_off, fb_on), 1, F_REPS, F_ROUNDS, F_WARMUP)
        fmt = lambda r: f"{r[0]:.3f} ({r[1]:.3f}-{r[2]:.3f})"
        say(f"{sname} | encode_frame ({ra.nbytes / 1e6:.1f} MB record) | {fmt(e)} | -")
        say(f"{sname} | chained flow from two images | {fmt(fi)} | -")
        say(f"{sname} | chained flow from two records | {fmt(fr)} | {fr[0] - fi[0]:+.3f} ms, x{fr[0] / fi[0]:.3f}")
        say(f"{sname} | compute_flow_fb | {fmt(f0)} | -")
        say(f"{sname} | compute_flow_fb, share_features | {fmt(f1)} | {f1[0] - f0[0]:+.3f} ms, x{f1[0] / f0[0]:.3f}")
        del prov, ra, rb, frames
        torch.cuda.empty_cache()


def bench_trackers(args, say):
    import bench
    from woft_amd import MultiFlowTracker
    warm = max(d for d in DELTAS[-1] if d is not None) + 2
    say(f"# MultiFlowTracker.track at 1080p: {ROUNDS} alternating rounds x {FRAMES} frames per tracker after {warm} warm-up frames each "
        f"(every delta has its source frame); raft_type 'weighted', {args.iters} flow iterations; host clock, one synchronise per round")
    say("# deltas | share_features off: ms per frame (min-max of the rounds) | on: ms per frame (min-max) | on - off | on / off")
    H, W = SIZES["1080p"]
    _, frames = bench.make_sequence(H, W, 0, bench.CLIP)
    trackers = []
    for deltas in DELTAS:
        for share in (False, True):
            trk = MultiFlowTracker(_provider(args), deltas=deltas, share_features=share)
            trk.init(frames[0])
            for t in range(1, warm + 1):
                trk.track(frames[t % len(frames)])
            trackers.append(((deltas, share), trk))
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in trackers}
    for r in range(ROUNDS):
        k = r % len(trackers)
        for key, trk in trackers[k:] + trackers[:k]:
            t0 = time.perf_counter()
            for _ in range(FRAMES):
                trk.track(frames[(trk.frame_index + 1) % len(frames)])
            torch.cuda.synchronize()
            ms[key].append((time.perf_counter() - t0) / FRAMES * 1e3)
    for deltas in DELTAS:
        off, on = ms[(deltas, False)], ms[(deltas, True)]
        say(f"{deltas!r} | {np.mean(off):.2f} ({min(off):.2f}-{max(off):.2f}) | {np.mean(on):.2f} ({min(on):.2f}-{max(on):.2f}) | "
            f"{np.mean(on) - np.mean(off):+.2f} ms | x{np.mean(on) / np.mean(off):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_features.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/bench_features.py on {torch.cuda.get_device_name(0)}")
    bench_kernels(args, say)
    bench_flows(args, say)
    bench_trackers(args, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
