"""What flow sampling, chaining and the forward-backward check cost:

    python tools/bench_flow_chain.py --out profiles/flow_chain_bench.txt

(1) the three kernels of csrc/flow_chain.hip at 1080p and 4K, in one process: HIP events around REPS back-to-back launches after a
    warm-up, the median of ROUNDS such measurements, next to a torch restatement of the same arithmetic on the device and next to
    the streaming floor -- the bytes the algorithm must move (chain: read fab, write fac, gather fbc once = 24 B per pixel; fb:
    20 B with one output, 24 B with both, 28 B counting a gather that misses twice; sampler: 8 B per point + 4 B per channel
    and point out + the gathered taps) over the HBM rate MEASURED on this part (6.29 TB/s float4 copy; 8.0 TB/s is the data
    sheet's).  Every launch works on another of N buffer sets that together exceed the 256 MiB Infinity Cache, so the figure is
    an HBM figure and not a cache one.
(2) the tracker with `fb_check` (WOFT_fbcheck.py, and the same with fb_beta = 1e12, which only drops flows that leave the frame)
    against the default one (WOFT.py), alternating rounds in one process on identical frames as tools/bench_window.py does; host
    clock around work that ends in a device synchronise.  The synthetic checkpoint's flow is no motion estimate: how many frames
    a tracker loses and how many correspondences the check keeps is reported, not judged.
No GPU: the tool fails, it has no fallback."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.bench_window import SIZES, centred_mask, run  # noqa: E402

ROUNDS, FRAMES, WARMUP = 4, 24, 8
K_REPS, K_ROUNDS, K_WARMUP = 24, 5, 24
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
CACHE_BYTES = 512 << 20               # buffer sets rotate over at least this much (twice the Infinity Cache)


def torch_sample(f, qx, qy):
    """The edge-exact sampler on the device in torch ops (fp32), at points already known to be valid or clamped."""
    _, h, w = f.shape
    x0, y0 = qx.floor().clamp(0, w - 1), qy.floor().clamp(0, h - 1)
    ax, ay = qx - x0, qy - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    flat = f.reshape(2, -1)
    g = lambda yy, xx: flat[:, (yy * w + xx).reshape(-1)].reshape(2, h, w)
    return (1 - ay) * ((1 - ax) * g(y0, x0) + ax * g(y0, x1)) + ay * ((1 - ax) * g(y1, x0) + ax * g(y1, x1))


def torch_landing(fab):
    _, h, w = fab.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=fab.device, dtype=torch.float32),
                            torch.arange(w, device=fab.device, dtype=torch.float32), indexing="ij")
    qx, qy = xs + fab[0], ys + fab[1]
    return qx, qy, (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)


def torch_chain(fab, fbc):
    qx, qy, valid = torch_landing(fab)
    return torch.where(valid, fab + torch_sample(fbc, qx, qy), torch.full_like(fab, float("nan")))


def torch_fb(fab, fba, alpha, beta):
    qx, qy, valid = torch_landing(fab)
    b = torch_sample(fba, qx, qy)
    e2 = ((fab + b) ** 2).sum(0)
    bound = alpha * ((fab ** 2).sum(0) + (b ** 2).sum(0)) + beta
    return torch.where(valid, e2.sqrt(), torch.full_like(e2, float("inf"))), (valid & (e2 <= bound)).float()


def timed(fn, n_sets):
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


def smooth_flow(h, w, seed, sign):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32),
                            indexing="ij")
    f = torch.stack([6.0 * torch.sin(xs / w * 2.3) + 2.0, -4.0 * torch.cos(ys / h * 1.9)]) * sign
    return (f + 0.3 * torch.randn(2, h, w, device="cuda", generator=g)).contiguous()


def bench_kernels(say):
    from woft_amd import ops
    say(f"# kernels: median over {K_ROUNDS} measurements of {K_REPS} back-to-back launches (HIP events) after {K_WARMUP} warm-up "
        f"launches, rotating over buffer sets of >= {CACHE_BYTES >> 20} MiB in all; floor = bytes / {HBM_MEASURED / 1e12:.2f} TB/s "
        f"(measured float4 copy rate; data sheet {HBM_SPEC / 1e12:.1f} TB/s)")
    say("# size | kernel | ms per launch (min-max) | torch restatement ms (min-max) | floor ms (bytes per pixel or point) | "
        "kernel / floor | torch / kernel")
    for sname, (h, w) in SIZES.items():
        n = h * w
        n_sets = max(2, -(-CACHE_BYTES // (n * 24)))
        fab = [smooth_flow(h, w, 10 + i, 1.0) for i in range(n_sets)]
        fba = [smooth_flow(h, w, 50 + i, -1.0) for i in range(n_sets)]
        out = [torch.empty(2, h, w, device="cuda") for _ in range(n_sets)]
        err, ok = [o[0] for o in out], [o[1] for o in out]
        qx = [(torch_landing(f)[0]).reshape(-1).contiguous() for f in fab]
        qy = [(torch_landing(f)[1]).reshape(-1).contiguous() for f in fab]
        rows = [
            ("woft_flow_chain", 24, lambda i: ops.flow_chain(fab[i], fba[i], out[i]), lambda i: torch_chain(fab[i], fba[i])),
            ("woft_flow_fb (err + ok)", 24, lambda i: ops.flow_fb(fab[i], fba[i], 0.01, 0.5, err[i], ok[i]),
             lambda i: torch_fb(fab[i], fba[i], 0.01, 0.5)),
            ("woft_flow_fb (ok only)", 20, lambda i: ops.flow_fb(fab[i], fba[i], 0.01, 0.5, None, ok[i], want_err=False),
             None),
            ("woft_sample_bilinear (2 channels, one point per pixel)", 24,
             lambda i: ops.sample_bilinear(fba[i], qx[i], qy[i], out[i].reshape(2, -1)),
             lambda i: torch_sample(fba[i], qx[i].reshape(h, w), qy[i].reshape(h, w))),
        ]
        for name, bpp, fn, ref in rows:
            k = timed(fn, n_sets)
            floor = n * bpp / HBM_MEASURED * 1e3
            t = timed(ref, n_sets) if ref is not None else None
            say(f"{sname} | {name} | {k[0]:.4f} ({k[1]:.4f}-{k[2]:.4f}) | "
                + (f"{t[0]:.4f} ({t[1]:.4f}-{t[2]:.4f})" if t else "-") + f" | {floor:.4f} ({bpp} B) | x{k[0] / floor:.2f} | "
                + (f"x{t[0] / k[0]:.1f}" if t else "-"))
        del fab, fba, out, err, ok, qx, qy
        torch.cuda.empty_cache()


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


def bench_trackers(args, say):
    import bench
    from woft_amd import synth
    sd = synth.make_state_dict(seed=7)
    say(f"# trackers: {ROUNDS} alternating rounds x {FRAMES} frames per tracker after {WARMUP} warm-up frames each; {args.iters} flow "
        f"iterations; device {torch.cuda.get_device_name(0)}")
    say("# size | per tracker: frames/s (min-max of the rounds) ms/frame, lost frames of the last round, mean share of the template's "
        "correspondences the check keeps | frame times over WOFT's")
    say("# (WOFT_fbcheck beta=1e12: the check only drops flows that leave the frame, so no frame is lost to the synthetic "
        "checkpoint's inconsistent flows and the row shows what the reverse flow itself costs; a lost frame also runs the local stage)")
    for sname in args.sizes:
        H, W = SIZES[sname]
        template, frames = bench.make_sequence(H, W, 0, bench.CLIP)
        mask = centred_mask(H, W, 2)
        n_mask = int((mask > 0).sum())
        trackers = [("WOFT", make_tracker("WOFT.py", sd, args.iters, template, mask)),
                    ("WOFT_fbcheck", make_tracker("WOFT_fbcheck.py", sd, args.iters, template, mask)),
                    ("WOFT_fbcheck beta=1e12", make_tracker("WOFT_fbcheck.py", sd, args.iters, template, mask, fb_beta=1e12))]
        for _, trk in trackers:
            run(trk, frames, 0, WARMUP)
        fps, res = {tag: [] for tag, _ in trackers}, {}
        for r in range(ROUNDS):
            first = WARMUP + r * FRAMES
            k = r % len(trackers)
            for tag, trk in trackers[k:] + trackers[:k]:
                if first % bench.CLIP:
                    bench.restart_clip(trk)
                dt, res[tag] = run(trk, frames, first, FRAMES)
                fps[tag].append(FRAMES / dt)
        parts = []
        for tag, _ in trackers:
            v = np.array(fps[tag])
            lost = sum(int(m.lost) for _, m in res[tag])
            s = f"{tag} {v.mean():7.1f} fps ({v.min():.1f}-{v.max():.1f}) {1000 / v.mean():6.2f} ms, {lost} of {FRAMES} lost"
            if tag != "WOFT":
                s += f", {100.0 * np.mean([m.n_kept for _, m in res[tag]]) / n_mask:.1f} % kept"
            parts.append(s)
        say(f"{sname} | " + " | ".join(parts) + " | "
            + " ".join(f"x{np.mean(fps['WOFT']) / np.mean(fps[tag]):.3f}" for tag, _ in trackers[1:]))
        del trackers
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=["1080p"], choices=list(SIZES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_flow_chain.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/bench_flow_chain.py on {torch.cuda.get_device_name(0)}")
    bench_kernels(say)
    bench_trackers(args, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
