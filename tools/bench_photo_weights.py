"""Times of the visibility weight map of the photometric refinement (woft_photo_weights, woft_amd.photo.photo_weight_map; DESIGN.md
section 30) in one process:

    python tools/bench_photo_weights.py --out profiles/photo_weights_bench.txt

  * one launch (with its memset of the counts when K > 0) at 1080p and 4K for radius 0 / 1 / 4 and K = 0 / 1 / 32 targets, REPS
    launches between device events, the median of ROUNDS rounds -- against its streaming floor, 16 B per pixel (8 B of planes and
    4 B of bits read, 4 B of map written) at the project's measured 6.29 TB/s streaming rate: the floor is DERIVED from shapes, not
    measured, and at K = 0 the bits are not read (12 B per pixel);
  * the same arithmetic in torch ops on the device (isfinite / compare / where, a max-pool of the negated map for the erosion, one
    masked sum per target), the same way;
  * WOFT_chained_photo_occl.py against WOFT_chained_photo.py -- the parent commit's tracker, the yardstick -- alternating rounds on
    identical frames, with the host's wait for the support counts.  The synthetic checkpoint's flow is no motion estimate, so
    besides the trackers as they are a second line overrules the fit in BOTH trackers with the sequence's own pose, the box
    corners moved by up to 1 px: the flows, the fold and woft_chain_tc still run, and the refinement runs on every frame.
No figure is fixed in advance.  No GPU: the tool fails, it has no fallback."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.bench_photo import SIZES, STREAM_BYTES_PER_S, centred_mask, perturbed  # noqa: E402

RADII, KS = (0, 1, 4), (0, 1, 32)
ROUNDS, REPS = 5, 50
T_ROUNDS, T_FRAMES, T_WARMUP = 4, 16, 4


def device_time_us(fn):
    """The median over ROUNDS of the device time per call of REPS calls between two events."""
    for _ in range(5):
        fn()
    us = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(1000.0 * e0.elapsed_time(e1) / REPS)
    return float(np.median(us)), min(us), max(us)


def torch_weight_map(cost, vis, bits, K, vis_thr, radius):
    """woft_photo_weights' gate map and counts in torch ops (planes of the template's size)."""
    raw = (torch.isfinite(cost) & (vis >= vis_thr)).to(torch.float32)
    wmap = raw if radius == 0 else -torch.nn.functional.max_pool2d(-raw[None, None], 2 * radius + 1, 1, radius)[0, 0]
    if K == 0:
        return wmap, None
    live = wmap > 0
    return wmap, torch.stack([(((bits >> t) & 1).bool() & live).sum() for t in range(K)]).to(torch.int32)


def bench_launch(sname, H, W, say):
    from woft_amd import photo
    from woft_amd.chained import pack_target_bits
    g = torch.Generator(device="cuda").manual_seed(3)
    cost = torch.rand((H, W), device="cuda", generator=g) * 3.0
    vis = torch.rand((H, W), device="cuda", generator=g)
    vis[H // 3:H // 2, W // 4:W // 2] = 0.0                      # (an occluder; elsewhere half the pixels pass at 0.5)
    rs = np.random.RandomState(5)
    for K in KS:
        bits = None
        if K:
            masks = []
            for t in range(K):                                   # (overlapping boxes of a quarter of each side)
                m = np.zeros((H, W), bool)
                y0, x0 = rs.randint(0, H - H // 4), rs.randint(0, W - W // 4)
                m[y0:y0 + H // 4, x0:x0 + W // 4] = True
                masks.append(m)
            bits = torch.from_numpy(pack_target_bits(masks).view(np.int32)).cuda()
        for radius in RADII:
            out = photo.photo_weight_map(cost, vis, (H, W), bits=bits, n_targets=K, erode=radius)
            ref = torch_weight_map(cost, vis, bits, K, 0.5, radius)
            assert torch.equal(out[0], ref[0]) and (K == 0 or torch.equal(out[1], ref[1])), "the kernel and the torch ops disagree"
            from woft_amd import ops
            call = lambda: ops.photo_weights(cost, vis, (0, 0, H, W), (H, W), bits, K, 0.5, 0, radius, out[0], out[1])
            us, lo, hi = device_time_us(call)
            tus, tlo, thi = device_time_us(lambda: torch_weight_map(cost, vis, bits, K, 0.5, radius))
            nbytes = H * W * (16 if K else 12)
            floor_us = 1e6 * nbytes / STREAM_BYTES_PER_S
            say(f"{sname} | radius {radius} | K {K:2d} | woft_photo_weights {us:8.2f} us ({lo:.2f}-{hi:.2f}) | floor, derived, not measured: "
                f"{nbytes / 1e6:.1f} MB / 6.29 TB/s = {floor_us:.2f} us | x{us / floor_us:.2f} of the floor | torch ops {tus:9.2f} us "
                f"({tlo:.2f}-{thi:.2f}) | torch / kernel x{tus / us:.1f}")


def bench_trackers(sname, frames, true, iters, say):
    from pytracking.utils.config import load_config
    from woft_amd import synth
    from woft_amd.planar import _Fit
    deltas = (None, 1)
    H, W = frames[0].shape[:2]
    mask = centred_mask(H, W, 4)
    ys, xs = np.nonzero(mask)
    box = (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))
    sd = synth.make_state_dict(seed=7)
    rs = np.random.RandomState(23)
    poses = [np.linalg.inv(perturbed(Ht, box, rs)) for Ht in true]                 # [frame of the clip]: frame -> template

    def make(name):
        conf = load_config(ROOT / "pytracking" / "configs" / name)
        conf.flow_config.model, conf.flow_config.iters, conf.chain_deltas = sd, iters, deltas
        trk = conf.tracker_class(conf)
        trk.init(frames[0], mask)
        return trk
    trackers = {"photo": make("WOFT_chained_photo.py"), "occl": make("WOFT_chained_photo_occl.py")}

    def overrule(trk):
        inner = trk._solve

        def solve(*a, **k):
            try:
                inner(*a, **k)                                   # (the selection and the fit still run)
            except AssertionError:
                pass
            trk.n_kept = max(int(trk.n_kept or 0), 4)
            return _Fit(H=poses[trk.multi.frame_index % len(poses)].copy(), success=True)
        trk._solve = solve
    nxt = lambda trk: frames[(trk.multi.frame_index + 1) % len(frames)]
    for label in ("trackers as they are", "the fit overruled with the sequence's pose, corners moved by <= 1 px"):
        if label != "trackers as they are":
            for trk in trackers.values():
                overrule(trk)
        for trk in trackers.values():
            for _ in range(T_WARMUP):
                trk.track(nxt(trk))
        ms = {name: [] for name in trackers}
        waits = {name: [] for name in trackers}
        refined = low = 0
        support = []
        for r in range(T_ROUNDS):
            for name in (("photo", "occl") if r % 2 == 0 else ("occl", "photo")):
                trk = trackers[name]
                w0, c0 = trk.host_wait_s, trk.photo_weights_wait_s
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = [trk.track(nxt(trk)) for _ in range(T_FRAMES)]
                torch.cuda.synchronize()
                ms[name].append(1000.0 * (time.perf_counter() - t0) / T_FRAMES)
                waits[name].append((1000.0 * (trk.host_wait_s - w0) / T_FRAMES, 1e6 * (trk.photo_weights_wait_s - c0) / T_FRAMES))
                if name == "occl":
                    done = [m.photo for _, m in res if getattr(m, "photo", None) is not None]
                    refined += sum(p.status != "LOW_SUPPORT" for p in done)
                    low += sum(p.status == "LOW_SUPPORT" for p in done)
                    support += [p.support for p in done]
        a, b = float(np.mean(ms["photo"])), float(np.mean(ms["occl"]))
        say(f"{sname} | deltas {deltas} | {label} | WOFT_chained_photo {a:6.2f} ms/frame ({min(ms['photo']):.2f}-{max(ms['photo']):.2f}), "
            f"host wait {np.mean([w for w, _ in waits['photo']]):.2f} ms/frame | WOFT_chained_photo_occl {b:6.2f} ms/frame "
            f"({min(ms['occl']):.2f}-{max(ms['occl']):.2f}), host wait {np.mean([w for w, _ in waits['occl']]):.2f} ms/frame of which "
            f"{np.mean([c for _, c in waits['occl']]):.1f} us/frame on the support counts | difference {b - a:+.3f} ms | refined {refined}, "
            f"low support {low} of {T_ROUNDS * T_FRAMES} frames, mean support {np.mean(support) if support else float('nan'):.3f}")
    del trackers
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trackers", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_photo_weights.py needs a GPU")
    import bench
    from woft_amd import synth
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/bench_photo_weights.py: device {torch.cuda.get_device_name(0)}; launches: gate mode, device events around {REPS} "
        f"calls, median (min-max) of {ROUNDS} rounds, planes of the template's size; trackers: one quarter-side centred mask, "
        f"{T_ROUNDS} alternating rounds x {T_FRAMES} frames after {T_WARMUP} warm-up frames, {args.iters} flow iterations, seeded "
        "random weights")
    for sname in args.sizes:
        H, W = SIZES[sname]
        bench_launch(sname, H, W, say)
        if not args.no_trackers:
            template, frames = bench.make_sequence(H, W, 0, bench.CLIP)
            true = [synth.seq_homography(t, H, W) for t in range(1, bench.CLIP + 1)]        # template -> frame
            bench_trackers(sname, [template] + list(frames), [np.eye(3)] + true, args.iters, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
