"""Forward + backward of RAFTWrapper.visibility_at() (csrc/mh_train.hip) at N = 500 and 2048 points on a
1080p flow for mask_head_structure [(128, 3), (128, 3)], against what a user had before it: the same head in plain float32 torch
ops on the device (F.conv2d over the same [fmap1 | warped fmap2] map, the convex upsampling at the points as gathers),
differentiated by torch autograd.  The restatement lives here, not in the product.  Loss = sum of the sigmoid visibilities times a
fixed random vector; one process, alternating rounds, HIP events around each round's calls.  Then the five GEMM-shaped launches
of one step on their own, next to their floor at the 155 TFLOP/s fp32 matrix rate.  The lines go to --out
(profiles/mh_train_bench.txt)."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import torch.nn.functional as F

from woft_amd import ops, presets, synth
from woft_amd.config import Config
from woft_amd.flow_provider import RAFTWrapper

STRUCTURE = [(128, 3), (128, 3)]
MATRIX_TFLOPS = 155.0


def torch_visibility_at(x, params, mask, pts, hf, wf, crop):
    """The head over the map x (1, 512, hf, wf), upsampled (x8, convex) at pts, sigmoid."""
    a = x
    for k in range(len(params) // 2 - 1):
        a = F.relu(F.conv2d(a, params[2 * k], params[2 * k + 1], padding=1))
    low = F.conv2d(a, params[-2], params[-1]).reshape(-1)
    X, Y = pts[:, 0].long() + crop[1], pts[:, 1].long() + crop[0]
    hc, wc, lane = Y >> 3, X >> 3, (Y & 7) * 8 + (X & 7)
    k = torch.arange(9, device=pts.device)
    s = torch.softmax(mask[(hc * wf + wc)[:, None], k[None] * 64 + lane[:, None]], dim=1)
    ny, nx = hc[:, None] + k[None] // 3 - 1, wc[:, None] + k[None] % 3 - 1
    inside = (ny >= 0) & (ny < hf) & (nx >= 0) & (nx < wf)
    v = torch.where(inside, 8 * low[torch.where(inside, ny * wf + nx, torch.zeros_like(ny))], torch.zeros((), device=low.device))
    return torch.sigmoid((s * v).sum(dim=1) / 8)


def _round(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def _stages(plan, params, rounds, reps):
    """The five GEMM-shaped launches of one step, each on its own on the plan's buffers -> lines."""
    t, hf, wf, P = plan._mh_train, plan.hf, plan.wf, plan.P
    w0, b0, w1, b1 = (p.detach() for p in params[:4])
    fwd = lambda w: w.permute(2, 3, 1, 0).reshape(9, w.shape[1], w.shape[0]).contiguous()
    wt0, wt1 = fwd(w0), fwd(w1)
    flip1 = w1.flip(2, 3).permute(2, 3, 0, 1).reshape(9, 128, 128).contiguous()
    a0, a1 = t["act"]
    gA, gB = t["g"]
    gw0, gb0, gw1, gb1 = torch.zeros_like(w0), torch.zeros_like(b0), torch.zeros_like(w1), torch.zeros_like(b1)
    f1, warped = plan.f1rows, plan.mh_warped.t
    stages = [("layer 0 forward   (512 -> 128)", 4608, lambda: ops.mh_train_conv(f1, warped, wt0, hf, wf, a0, bias=b0)),
              ("layer 1 forward   (128 -> 128)", 1152, lambda: ops.mh_train_conv(a0, None, wt1, hf, wf, a1, bias=b1)),
              ("layer 1 weight gradient       ", 1152, lambda: ops.mh_wgrad(gA, a0, None, hf, wf, t["ws"], gw1, gb1)),
              ("layer 1 data gradient         ", 1152, lambda: ops.mh_train_conv(gA, None, flip1, hf, wf, gB, gate=a0)),
              ("layer 0 weight gradient       ", 4608, lambda: ops.mh_wgrad(gB, f1, warped, hf, wf, t["ws"], gw0, gb0))]
    lines, total, floor_total = [], 0.0, 0.0
    for name, k, fn in stages:
        fn()
        ms = sorted(_round(fn, reps) for _ in range(rounds))[rounds // 2]
        floor = 2.0 * P * k * 128 / (MATRIX_TFLOPS * 1e9)
        total, floor_total = total + ms, floor_total + floor
        lines.append(f"  {name} {ms:7.3f} ms | floor {floor:.3f} ms | {2.0 * P * k * 128 / ms / 1e9:6.1f} TFLOP/s")
    lines.append(f"  the five launches together     {total:7.3f} ms | floor {floor_total:.3f} ms at {MATRIX_TFLOPS:.0f} TFLOP/s")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[500, 2048])
    ap.add_argument("--size", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="file the lines are written to (profiles/mh_train_bench.txt)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the training benchmark needs the MI355X: nothing is measured without it"
    H, W = args.size
    c = Config()
    c.of_class, c.raft_type, c.class_params = RAFTWrapper, "weighted_masked", Config()
    c.class_params.small = c.class_params.mixed_precision = c.class_params.alternate_corr = False
    c.class_params.weight_head_structure = [(128, 3)] * 3
    c.class_params.mask_estimation, c.class_params.mask_head_structure = True, STRUCTURE
    c.model, c.iters, c.padding_mode = synth.make_state_dict(seed=0, mask_head_structure=STRUCTURE), 4, "RAFT"
    c.weights_postprocessing_fn = None
    prov = RAFTWrapper(c)
    template = synth.make_template(H, W)
    prov.compute_flow(template, synth.make_frame(template, 3), mode="flow")
    plan, crop = prov._last.wh
    hf, wf, P = plan.hf, plan.wf, plan.P
    params = list(prov.mask_head_parameters().values())
    x = torch.cat([plan.f1rows[:P, :256], plan.mh_warped.t[:P, :256]], 1).reshape(hf, wf, 512).permute(2, 0, 1)[None].contiguous()
    mask = plan.mask.t
    lines = [f"forward + backward of sum(g * visibility_at(pts, do_sigmoid=True)) into the parameters of the MaskHead {STRUCTURE} on "
             f"a {H} x {W} flow ({hf} x {wf} map; precision {prov.precision}); {args.rounds} alternating rounds of {args.reps} calls "
             "each after one warm-up round, ms per call: median (min - max)"]
    for n in args.n:
        idx = np.unique(np.minimum(np.round(H * W * presets.sobol_points(n)).astype(np.int64), H * W - 1))
        pts = torch.from_numpy(np.stack([idx % W, idx // W], 1).astype(np.float32)).cuda()
        g = torch.randn(pts.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        grads = {}

        def hip():
            for p in params:
                p.grad = None
            (prov.visibility_at(pts, do_sigmoid=True) * g).sum().backward()
            grads["hip"] = [p.grad for p in params]

        def eager():
            for p in params:
                p.grad = None
            (torch_visibility_at(x, params, mask, pts, hf, wf, crop) * g).sum().backward()
            grads["torch"] = [p.grad for p in params]
        sides = [("hip", hip), ("torch", eager)]
        t = {k: [] for k, _ in sides}
        for r in range(args.rounds + 1):
            for label, fn in sides:
                ms = _round(fn, args.reps)
                if r > 0:                            # (round 0 warms both up)
                    t[label].append(ms)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        agree = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads["hip"], grads["torch"]))
        lines.append(f"N={pts.shape[0]:5d} | HIP visibility_at fwd + bwd {med['hip']:8.2f} ms ({min(t['hip']):.2f} - "
                     f"{max(t['hip']):.2f}) | float32 torch head + autograd {med['torch']:8.2f} ms ({min(t['torch']):.2f} - "
                     f"{max(t['torch']):.2f}) | torch / HIP = {med['torch'] / med['hip']:.2f} | largest relative gradient difference "
                     f"{agree:.1e}")
        print(lines[-1], flush=True)
    lines.append("the five GEMM-shaped launches of one step on their own (median of the rounds):")
    lines += _stages(plan, params, args.rounds, args.reps)
    print("\n".join(lines[-7:]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
