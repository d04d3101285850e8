"""Frames/s of the search-window tracker (WOFTWindow, pytracking/configs/WOFT_window.py, margin 0.25) against the full-frame
tracker (YAOFTrackerSingleControl, WOFT.py) on identical frames, in one process:

    python tools/bench_window.py --out profiles/window_bench.txt              # the tracker lines
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_window.py --kernels
    python tools/bench_window.py --kernel-stats <dir> --out profiles/window_bench.txt --append      # the kernel lines

The sequences are bench.py's (woft_amd.synth, 1080p and 4K, shipped arithmetic, 12 flow iterations); the masks are centred
rectangles covering 1/4, 1/16 and 1/64 of the frame.  Per size and mask both trackers are warmed up, then timed in ROUNDS
alternating rounds of FRAMES frames each (host clock around work that ends in a device synchronise), so clock drift and
neighbours on the host hit both; the spread of the rounds is printed next to the mean.  A lost-frame line times frames whose
re-detection verdict is overruled (global flow + local flow).  No GPU: the tool fails, it has no fallback."""
import argparse
import csv
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ROUNDS, FRAMES, WARMUP, LOST_FRAMES = 4, 24, 8, 12
SIZES = {"1080p": (1080, 1920), "4K": (2160, 3840)}
MASKS = {"1/4": 2, "1/16": 4, "1/64": 8}          # mask side = frame side / k


def centred_mask(H, W, k):
    m = np.zeros((H, W), np.uint8)
    h, w = H // k, W // k
    m[(H - h) // 2:(H - h) // 2 + h, (W - w) // 2:(W - w) // 2 + w] = 255
    return m


def make_tracker(cfg, sd, iters, template, mask):
    from pytracking.utils.config import load_config
    conf = load_config(ROOT / "pytracking" / "configs" / cfg)
    conf.flow_config.model = sd
    conf.flow_config.iters = iters
    conf.flow_config.padding_mode = "RAFT"           # (both trackers: the window's sides are no multiples of 8)
    trk = conf.tracker_class(conf)
    trk.init(template, mask)
    return trk


def run(trk, frames, first, n, force_lost=False):
    """-> (seconds, results) for frames[first : first + n] of the clip (pose restarted at the clip's start, as bench.py does)."""
    import bench
    inner = type(trk)._global_stage.__get__(trk)

    def overruled(frame, prewarp_H):
        fit = inner(frame, prewarp_H)
        fit.success = False
        return fit
    if force_lost:
        trk._global_stage = overruled
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = []
    for i in range(first, first + n):
        if i % bench.CLIP == 0:
            bench.restart_clip(trk)
        res.append(trk.track(frames[i % bench.CLIP]))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if force_lost:
        del trk._global_stage
    return dt, res


def corners_gap(Ha, Hb, mask):
    from woft_amd.window import Box
    b = Box.from_mask(mask > 0)
    c = np.array([[b.tl_x, b.tl_y, 1], [b.br_x, b.tl_y, 1], [b.br_x, b.br_y, 1], [b.tl_x, b.br_y, 1.0]]).T
    pa, pb = np.linalg.inv(Ha) @ c, np.linalg.inv(Hb) @ c
    return float(np.abs(pa[:2] / pa[2] - pb[:2] / pb[2]).max())


def bench_trackers(args, say):
    import bench
    from woft_amd import synth
    sd = synth.make_state_dict(seed=7)
    say(f"# tools/bench_window.py: {ROUNDS} alternating rounds x {FRAMES} frames per tracker after {WARMUP} warm-up frames each; "
        f"{args.iters} flow iterations; device {torch.cuda.get_device_name(0)}")
    say("# size mask | full-frame tracker: frames/s (min-max of the rounds) ms/frame | window tracker: the same | window crop | "
        "ratio window/full | poses: largest corner distance between the two trackers [px]")
    # (that last column is reported, not judged: the synthetic checkpoint's flow is no motion estimate and the two trackers see
    #  different pixels; what WOFTWindow computes is pinned by the golden tests)
    for sname in args.sizes:
        H, W = SIZES[sname]
        template, frames = bench.make_sequence(H, W, 0, bench.CLIP)
        for mname, k in MASKS.items():
            mask = centred_mask(H, W, k)
            full = make_tracker("WOFT.py", sd, args.iters, template, mask)
            win = make_tracker("WOFT_window.py", sd, args.iters, template, mask)
            rows, cols = win._rect[2], win._rect[3]
            run(full, frames, 0, WARMUP)
            run(win, frames, 0, WARMUP)
            fps = {"full": [], "win": []}
            gap = 0.0
            for r in range(ROUNDS):
                first = WARMUP + r * FRAMES
                order = (("full", full), ("win", win)) if r % 2 == 0 else (("win", win), ("full", full))
                res = {}
                for tag, trk in order:
                    if first % bench.CLIP:                 # both start a round from the same pose: the clip's, restarted
                        bench.restart_clip(trk)
                    dt, res[tag] = run(trk, frames, first, FRAMES)
                    fps[tag].append(FRAMES / dt)
                gap = max([gap] + [corners_gap(a[0], b[0], mask) for a, b in zip(res["full"], res["win"])])
                lost = sum(int(m.lost) for _, m in res["full"]), sum(int(m.lost) for _, m in res["win"])
            f, w = np.array(fps["full"]), np.array(fps["win"])
            say(f"{sname} {mname} | full {f.mean():7.1f} fps ({f.min():.1f}-{f.max():.1f}) {1000 / f.mean():6.2f} ms | "
                f"window {w.mean():7.1f} fps ({w.min():.1f}-{w.max():.1f}) {1000 / w.mean():6.2f} ms | {rows} x {cols} of {H} x {W} | "
                f"x{w.mean() / f.mean():.2f} | {gap:.3f} px, lost frames in the last round {lost[0]} / {lost[1]}")
            # lost frames: both flows of a frame (template -> window, frame t-1 -> t on the carried mask's box)
            for trk in (full, win):
                bench.restart_clip(trk)
                run(trk, frames, 0, 4, force_lost=True)
            t = {}
            for tag, trk in (("full", full), ("win", win)):
                bench.restart_clip(trk)
                dt, _ = run(trk, frames, 0, LOST_FRAMES, force_lost=True)
                t[tag] = 1000 * dt / LOST_FRAMES
            lb = win.local_search_bbox
            say(f"{sname} {mname} | lost frames ({LOST_FRAMES}, every verdict overruled): full {t['full']:6.2f} ms/frame, window "
                f"{t['win']:6.2f} ms/frame, last local window {lb.crop_rect()[2]} x {lb.crop_rect()[3]}, plans kept "
                f"{len(win.flower.engine._plans)}")
            del full, win
            torch.cuda.empty_cache()


def bench_kernels(args, say):
    """The glue kernels alone, for a kernel trace: windowed warp against full warp + slice, rectangle copy against the torch slice,
    bounding box (fused with the mask warp) against warp + torch reductions.  1080p, the 1/4 mask's window."""
    from woft_amd import ops, synth
    from woft_amd.window import Box, search_box
    H, W = SIZES["1080p"]
    img = torch.from_numpy(synth.make_template(H, W, seq_id=0)).cuda()
    mask = torch.from_numpy(centred_mask(H, W, 2)).cuda()
    rect = search_box(Box.from_mask(mask.cpu().numpy()), 0.25, W, H).crop_rect()
    y0, x0, rows, cols = rect
    Hm = synth.seq_homography(5, H, W)
    full, fvalid = torch.empty_like(img), torch.empty((H, W), dtype=torch.uint8, device="cuda")
    out, valid = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda"), torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
    warped = torch.empty_like(mask)
    for _ in range(args.reps):
        ops.warp_perspective_u8(img, Hm, full, fvalid)                      # warp_kernel + two strided copies
        a = full[y0:y0 + rows, x0:x0 + cols].contiguous()
        b = fvalid[y0:y0 + rows, x0:x0 + cols].contiguous()
        ops.warp_perspective_window_u8(img, Hm, rect, out, valid)           # warp_window_kernel
        c = img[y0:y0 + rows, x0:x0 + cols].contiguous()                    # torch's strided copy (3 channels)
        d = ops.crop_u8(img, rect)                                          # crop_kernel
        ops.mask_bbox(mask, Hmat=Hm, warped=warped)                         # warp_mask_bbox_kernel
        ops.mask_bbox(mask)                                                 # mask_bbox_kernel
    torch.cuda.synchronize()
    assert torch.equal(a, out) and torch.equal(b, valid) and torch.equal(c, d)
    say(f"# kernel pass done: {args.reps} repetitions, 1080p, window {rows} x {cols}")


def kernel_stats(args, say):
    files = sorted(Path(args.kernel_stats).rglob("*kernel_stats.csv"))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {args.kernel_stats}")
    say("# kernel times (rocprofv3 --kernel-trace --stats of `tools/bench_window.py --kernels`, a run of its own; 1080p, the 1/4 "
        "mask's window): name | calls | average ns | total ns")
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            if any(s in name for s in ("warp_kernel", "warp_window_kernel", "crop_kernel", "mask_bbox_kernel", "elementwise", "copy")):
                say(f"{name[:110]} | {row.get('Calls')} | {float(row.get('AverageNs', 0)):.0f} | {row.get('TotalDurationNs')}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if args.kernel_stats:
        kernel_stats(args, say)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("tools/bench_window.py needs a GPU")
        (bench_kernels if args.kernels else bench_trackers)(args, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a" if args.append else "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
