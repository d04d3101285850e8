"""Times of the batched photometric refinement (woft_amd.photo.PhotoTemplateMulti, woft_photo_refine_multi)
against its yardstick, the loop of K single refinements, in one process:

    python tools/bench_photo_multi.py --out profiles/photo_multi_bench.txt

  * at 1080p and 4K, K = 1, 4, 16, 32 rectangular masks of 1/16 of each frame side on a grid: one PhotoTemplateMulti.refine call
    (10 iterations, including its one read; host clock) against the loop of K PhotoTemplate.refine calls on the same masks and
    poses, alternating, the median of ROUNDS rounds of REPS calls -- with the default eps (the refinements stop early: the mean
    number of evaluated iterates is printed) and with eps = 0 (all 11);
  * WOFT_chained_multi_photo.py against WOFT_chained_multi.py at K = 4, alternating rounds on identical frames.  The synthetic
    checkpoint's flow is no motion estimate, so besides the trackers as they are (the refined-target count says how often the stage
    ran at all) a second line overrules every target's fit in BOTH trackers with the sequence's own pose, the target's box corners
    moved by up to 1 px: the flows, the fold and the planar block still run, and the refinement starts from a pose as a trained
    network would leave it.
No figure is fixed in advance.  No GPU: the tool fails, it has no fallback."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.bench_photo import SIZES, perturbed  # noqa: E402

KS = (1, 4, 16, 32)
ROUNDS, REPS = 5, 20
T_ROUNDS, T_FRAMES, T_WARMUP = 3, 16, 4


def grid_masks(H, W, K):
    """K rectangles of 1/16 of each frame side on an 8 x 4 grid around the frame's centre -> [(h, w) uint8], their boxes."""
    h, w = H // 16, W // 16
    masks, boxes = [], []
    for t in range(K):
        gy, gx = divmod(t, 8)
        y0, x0 = H // 2 + (gy - 2) * (h + h // 2), W // 2 + (gx - 4) * (w + w // 4)
        m = np.zeros((H, W), np.uint8)
        m[y0:y0 + h, x0:x0 + w] = 255
        masks.append(m)
        boxes.append((x0, y0, x0 + w - 1, y0 + h - 1))
    return masks, boxes


def bench_refinements(sname, template, frame, true, say):
    from woft_amd.photo import PhotoTemplate, PhotoTemplateMulti
    H, W = template.shape[:2]
    d_t, d_f = ((a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).cuda() for a in (template, frame))
    rs = np.random.RandomState(17)
    for K in KS:
        masks, boxes = grid_masks(H, W, K)
        Ws = np.stack([perturbed(true, b, rs) for b in boxes])
        multi = PhotoTemplateMulti(d_t, masks)
        singles = [PhotoTemplate(d_t, m) for m in masks]
        for eps, label in ((1e-3, "default eps 1e-3"), (0.0, "eps 0")):
            kw = dict(iters=10, eps=eps)
            fns = {"batched": lambda: multi.refine(d_f, Ws, **kw), "loop": lambda: [s.refine(d_f, Ws[t], **kw) for t, s in enumerate(singles)]}
            for fn in fns.values():
                for _ in range(3):
                    fn()
            ms = {name: [] for name in fns}
            for r in range(ROUNDS):
                for name in (("batched", "loop") if r % 2 == 0 else ("loop", "batched")):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(REPS):
                        fns[name]()
                    ms[name].append(1000.0 * (time.perf_counter() - t0) / REPS)
            _, infos = multi.refine(d_f, Ws, **kw)
            evaluated = float(np.mean([len(i.cost) for i in infos]))
            a, b = float(np.median(ms["batched"])), float(np.median(ms["loop"]))
            say(f"{sname} | K {K:2d} | {label:16s} | batched {a:7.3f} ms ({min(ms['batched']):.3f}-{max(ms['batched']):.3f}) | loop of {K} "
                f"{b:7.3f} ms ({min(ms['loop']):.3f}-{max(ms['loop']):.3f}) | loop / batched x{b / a:.2f} | {evaluated:.1f} evaluated "
                f"iterates per target, statuses {sorted({i.status for i in infos})}")
        del multi, singles


def bench_trackers(sname, frames, true, iters, say):
    import bench
    from pytracking.utils.config import load_config
    from woft_amd import synth
    from woft_amd.planar import _Fit
    K, deltas = 4, (None, 1)
    H, W = frames[0].shape[:2]
    masks, boxes = grid_masks(H, W, K)
    sd = synth.make_state_dict(seed=7)
    rs = np.random.RandomState(23)
    poses = [[np.linalg.inv(perturbed(Ht, b, rs)) for b in boxes] for Ht in true]          # [frame of the clip][target]: frame -> template

    def make(name):
        conf = load_config(ROOT / "pytracking" / "configs" / name)
        conf.flow_config.model, conf.flow_config.iters, conf.chain_deltas = sd, iters, deltas
        trk = conf.tracker_class(conf)
        trk.init(frames[0], masks)
        return trk
    trackers = {"plain": make("WOFT_chained_multi.py"), "photo": make("WOFT_chained_multi_photo.py")}

    def overrule(trk):
        inner = type(trk)._planar_batched.__get__(trk)

        def planar(out, input_img):
            at = poses[trk.multi.frame_index % len(poses)]               # (the frame just folded)
            return [(_Fit(H=at[t].copy(), success=True), sel, max(int(kept or 0), 4), counts)
                    for t, (_, sel, kept, counts) in enumerate(inner(out, input_img))]
        trk._planar_batched = planar
    nxt = lambda trk: frames[(trk.multi.frame_index + 1) % len(frames)]
    for label in ("trackers as they are", "every target's fit overruled with the sequence's pose, corners moved by <= 1 px"):
        if label != "trackers as they are":
            for trk in trackers.values():
                overrule(trk)
        for trk in trackers.values():
            for _ in range(T_WARMUP):
                trk.track(nxt(trk))
        ms = {name: [] for name in trackers}
        refined = evaluated = 0
        for r in range(T_ROUNDS):
            for name in (("plain", "photo") if r % 2 == 0 else ("photo", "plain")):
                trk = trackers[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = [trk.track(nxt(trk)) for _ in range(T_FRAMES)]
                torch.cuda.synchronize()
                ms[name].append(1000.0 * (time.perf_counter() - t0) / T_FRAMES)
                if name == "photo":
                    done = [m.photo for _, metas in res for m in metas if getattr(m, "photo", None) is not None]
                    refined += len(done)
                    evaluated += sum(p.iterates for p in done)
        a, b = float(np.mean(ms["plain"])), float(np.mean(ms["photo"]))
        say(f"{sname} | K {K}, deltas {deltas} | {label} | WOFT_chained_multi {a:6.2f} ms/frame ({min(ms['plain']):.2f}-{max(ms['plain']):.2f}) | "
            f"WOFT_chained_multi_photo {b:6.2f} ms/frame ({min(ms['photo']):.2f}-{max(ms['photo']):.2f}) | difference {b - a:+.3f} ms | "
            f"refined {refined} of {T_ROUNDS * T_FRAMES * K} target frames, {evaluated / max(refined, 1):.1f} evaluated iterates each")
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
        raise SystemExit("tools/bench_photo_multi.py needs a GPU")
    import bench
    from woft_amd import synth
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"# tools/bench_photo_multi.py: device {torch.cuda.get_device_name(0)}; K masks of 1/16 of each frame side; refinements: 10 "
        f"iterations, host clock including the read(s), median (min-max) of {ROUNDS} alternating rounds x {REPS} calls; trackers: "
        f"{T_ROUNDS} alternating rounds x {T_FRAMES} frames after {T_WARMUP} warm-up frames, {args.iters} flow iterations, seeded "
        "random weights")
    for sname in args.sizes:
        H, W = SIZES[sname]
        template, frames = bench.make_sequence(H, W, 0, bench.CLIP)
        true = [synth.seq_homography(t, H, W) for t in range(1, bench.CLIP + 1)]            # template -> frame
        bench_refinements(sname, template, frames[2], true[2], say)
        if not args.no_trackers:
            bench_trackers(sname, [template] + list(frames), [np.eye(3)] + true, args.iters, say)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
