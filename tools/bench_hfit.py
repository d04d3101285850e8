"""H fit on every pixel of a frame (the configs without a subsampler): N = H*W correspondences through the
streaming multi-workgroup fit vs the single-workgroup kernel, weighted LSq and IRLS (6 solves).

`--batch B [B ...]` times the batched fit instead: ONE woft_hfit_batched launch for a (B, N, 2) problem against the
per-element loop the public estimators ran before it existed (B ops.hfit calls on the slices of the batch), N = 500 by
default, weighted LSq and IRLS Huber (6 solves); same process, same operands, alternating rounds, HIP events around each
round's calls; the two must return the same bits.  The lines go to --out (profiles/hfit_batched_bench.txt)."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from woft_amd import _lib, ops
from tools.bench_conv import bench


def _round(fn, reps):
    """microseconds per call of `reps` back-to-back calls (HIP events around the lot, ending in a synchronise)."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def bench_batched(batches, n, rounds, reps, out_path):
    assert torch.cuda.is_available(), "the batched-fit benchmark needs the MI355X: nothing is measured without it"
    lines = [f"woft_hfit_batched (one launch) against the loop of B woft_hfit launches, N = {n}; {rounds} alternating rounds of "
             f"{reps} calls each after one warm-up round, us per (B, N, 2) call: median of the rounds (min - max)"]
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in batches:
        a = torch.stack([torch.rand(B, n, device="cuda", generator=g) * 1700 + 100,
                         torch.rand(B, n, device="cuda", generator=g) * 920 + 80], -1).contiguous()
        b = (a * 1.01 + torch.tensor([3.0, -2.0], device="cuda") + torch.randn(B, n, 2, device="cuda", generator=g) * 0.3).contiguous()
        w = (torch.rand(B, n, device="cuda", generator=g) * 0.9 + 0.1).contiguous()
        Hb, sb = torch.zeros(B, 9, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        Hl, sl = torch.zeros(B, 9, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        for name, kw in (("weighted LSq", dict()), ("IRLS Huber, 6 solves", dict(reweight=2, huber_k=0.01, n_irls=5))):
            def batched():
                ops.hfit_batched(a, b, w, Hb, sb, **kw)

            def loop():                               # the per-element loop of homography._fit before the batched launch
                for e in range(B):
                    ops.hfit(a[e].float().contiguous(), b[e].float().contiguous(), w[e].float().reshape(-1).contiguous(),
                             Hl[e].view(9), sl[e:e + 1], **kw)
            t = {"batched": [], "loop": []}
            for r in range(rounds + 1):
                for label, fn in (("batched", batched), ("loop", loop)):
                    us = _round(fn, reps)
                    if r > 0:                        # (round 0 warms both up)
                        t[label].append(us)
            same = torch.equal(Hb, Hl) and torch.equal(sb, sl) and int(sb.abs().sum()) == 0
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            lines.append(f"B={B:3d} {name:22s} | batched {med['batched']:8.1f} us ({min(t['batched']):.1f} - {max(t['batched']):.1f})"
                         f" | loop {med['loop']:8.1f} us ({min(t['loop']):.1f} - {max(t['loop']):.1f})"
                         f" | loop / batched = {med['loop'] / med['batched']:.2f} | same bits: {same}")
            print(lines[-1], flush=True)
            assert same, "the batched launch and the per-element loop disagree"
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=None, help="time the batched fit at these batch sizes (e.g. 8 64)")
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None, help="with --batch: file the lines are written to (profiles/hfit_batched_bench.txt)")
    args = ap.parse_args()
    if args.batch:
        return bench_batched(args.batch, args.n, args.rounds, args.reps, args.out)
    lib = _lib.load()
    for (H, W) in ((1080, 1920), (2160, 3840), (128, 160), (64, 64), (32, 64)):
        n = H * W
        idx = torch.arange(n, device="cuda")
        a = torch.stack([idx % W, idx // W], 1).float().contiguous()
        b = (a * 1.01 + torch.tensor([3.0, -2.0], device="cuda") + torch.randn(n, 2, device="cuda") * 0.3).contiguous()
        w = (torch.rand(n, device="cuda") * 0.9 + 0.1).contiguous()
        Hd, st = torch.zeros(9, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = ops.hfit_ws()
        for name, rew, nir in (("weighted LSq", 0, 0), ("IRLS Huber, 6 solves", 2, 5), ("IRLS L1, 6 solves", 1, 5)):
            row = f"{H}x{W} N={n:8d} {name:22s}"
            for label, wsp in (("streaming", ws.data_ptr()), ("one workgroup", None)):
                if wsp is None and n > 3_000_000:
                    continue
                fn = lambda: _lib.check(lib.woft_hfit(a.data_ptr(), b.data_ptr(), w.data_ptr(), n, None, rew, 0.01, nir, wsp,
                                                      Hd.data_ptr(), st.data_ptr(), _lib.stream_ptr()), "woft_hfit")
                ms = bench(fn, reps=7)
                passes = (2 + (nir + 1 if rew else 1))
                row += f" | {label}: {ms * 1e3:9.1f} us ({20.0 * n * passes / ms / 1e6:7.1f} GB/s algorithmic)"
            print(row, flush=True)


if __name__ == "__main__":
    main()
