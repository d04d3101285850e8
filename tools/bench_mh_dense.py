"""Forward + backward of RAFTWrapper.visibility_map() (csrc/upsample_bwd.hip + csrc/mh_train.hip) on a 1080p
flow for mask_head_structure [(128, 3), (128, 3)] with a dense BCE-with-logits loss, next to visibility_at() at N = 2048 points
(tools/bench_mh_train.py's loss) and to what a user had before: the same head and the same dense x8 convex upsampling in plain
float32 torch ops on the device (F.conv2d, F.unfold, softmax), differentiated by torch autograd.  The restatement lives here, not in
the product.  One process, alternating rounds, HIP events around each round's calls.  Then woft_convex_upsample_bwd on its own,
next to its streaming floor: the bytes it must move over the 6.29 TB/s this project measured.  The lines go to --out
(profiles/mh_train_dense_bench.txt)."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import torch.nn.functional as F

from bench_mh_train import STRUCTURE, _round, torch_visibility_at  # noqa: F401
from woft_amd import ops, presets, synth
from woft_amd.config import Config
from woft_amd.flow_provider import RAFTWrapper

STREAM_TBPS = 6.29


def torch_visibility_map(x, params, mask, hf, wf, crop, h, w):
    """The head over the map x (1, 512, hf, wf), upsampled (x8, convex) everywhere as the reference writes it, cropped; logits."""
    a = x
    for k in range(len(params) // 2 - 1):
        a = F.relu(F.conv2d(a, params[2 * k], params[2 * k + 1], padding=1))
    low = F.conv2d(a, params[-2], params[-1])
    m = torch.softmax(mask[:hf * wf, :576].t().reshape(1, 1, 9, 8, 8, hf, wf), dim=2)
    up = F.unfold(8 * low, [3, 3], padding=1).view(1, 1, 9, 1, 1, hf, wf)
    up = torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(8 * hf, 8 * wf) / 8
    return up[crop[0]:crop[0] + h, crop[1]:crop[1] + w]


def adjoint_bytes(P, h, w):
    """What woft_convex_upsample_bwd must move with do_sigmoid: the mask and g_up once, wlow, the 9 P partials out and in, g_wlow."""
    return 4 * (576 * P + h * w + P + 2 * 9 * P + P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--size", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="file the lines are written to (profiles/mh_train_dense_bench.txt)")
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
    gen = torch.Generator(device="cuda").manual_seed(1)
    target = (torch.rand(H, W, device="cuda", generator=gen) > 0.5).float()
    valid = torch.rand(H, W, device="cuda", generator=gen) > 0.1
    idx = np.unique(np.minimum(np.round(H * W * presets.sobol_points(args.n)).astype(np.int64), H * W - 1))
    pts = torch.from_numpy(np.stack([idx % W, idx // W], 1).astype(np.float32)).cuda()
    g = torch.randn(pts.shape[0], device="cuda", generator=gen)
    grads = {}

    def zero():
        for p in params:
            p.grad = None

    def dense():
        zero()
        F.binary_cross_entropy_with_logits(prov.visibility_map()[valid], target[valid]).backward()
        grads["map"] = [p.grad for p in params]

    def at():
        zero()
        (prov.visibility_at(pts, do_sigmoid=True) * g).sum().backward()

    def eager():
        zero()
        F.binary_cross_entropy_with_logits(torch_visibility_map(x, params, mask, hf, wf, crop, H, W)[valid], target[valid]).backward()
        grads["torch"] = [p.grad for p in params]
    sides = [("map", dense), ("at", at), ("torch", eager)]
    t = {k: [] for k, _ in sides}
    for r in range(args.rounds + 1):
        for label, fn in sides:
            ms = _round(fn, args.reps)
            if r > 0:                            # (round 0 warms all three up)
                t[label].append(ms)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    agree = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads["map"], grads["torch"]))
    span = lambda k: f"{med[k]:8.2f} ms ({min(t[k]):.2f} - {max(t[k]):.2f})"
    lines = [f"forward + backward into the parameters of the MaskHead {STRUCTURE} on a {H} x {W} flow ({hf} x {wf} map; precision "
             f"{prov.precision}); {args.rounds} alternating rounds of {args.reps} calls each after one warm-up round, ms per call: "
             "median (min - max)",
             f"HIP visibility_map, BCE-with-logits on {int(valid.sum())} valid pixels          {span('map')}",
             f"HIP visibility_at, N = {pts.shape[0]}, sum(g * sigmoid visibility)            {span('at')}",
             f"float32 torch head + dense upsampling + autograd, the same BCE loss {span('torch')} | torch / HIP map = "
             f"{med['torch'] / med['map']:.2f} | largest relative gradient difference {agree:.1e}"]
    # the dense adjoint on its own, on the plan's buffers (the working set, 83 MB, fits the 256 MiB Infinity Cache: back-to-back
    # calls may be served from it, which a training step's single call is not)
    tb = plan._mh_train
    g_up = torch.randn(H * W, device="cuda", generator=gen)
    for sig in (False, True):
        fn = lambda: ops.convex_upsample_bwd(g_up, mask, tb["low"], hf, wf, crop, H, W, tb["up"], tb["g_low"], do_sigmoid=sig)
        fn()
        ts = sorted(_round(fn, args.kernel_reps) for _ in range(args.rounds))
        floor_us = adjoint_bytes(P, H, W) / (STREAM_TBPS * 1e12) * 1e6
        us = ts[len(ts) // 2] * 1e3
        lines.append(f"woft_convex_upsample_bwd alone (both launches), do_sigmoid={sig}: {us:7.1f} us per call (min {ts[0] * 1e3:.1f}; "
                     f"{args.kernel_reps} back-to-back calls per round, operands may stay in the Infinity Cache) | "
                     f"{adjoint_bytes(P, H, W) / 1e6:.1f} MB -> derived floor {floor_us:.1f} us at {STREAM_TBPS} TB/s | "
                     f"{us / floor_us:.2f} x the floor")
    print("\n".join(lines), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
