"""Forward + backward of RAFTWrapper.weights_at() (csrc/wh_train.hip) at N = 500 and 2048 points on a
1080p flow, against what a user had before it: the same head in plain float32 torch ops on the device (F.conv2d on the same
compacted windows, the convex upsampling at the points as gathers), differentiated by torch autograd.  The restatement lives
here, not in the product.  Loss = sum of the sigmoid weights times a fixed random vector; one process, alternating rounds, HIP
events around each round's calls.  The lines go to --out (profiles/wh_train_bench.txt)."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import torch.nn.functional as F

from woft_amd import presets, synth
from woft_amd.config import Config
from woft_amd.flow_provider import RAFTWrapper


def torch_weights_at(x5, params, index, mask, pts, hf, wf, crop):
    """The head on the windows x5 (n_win, 5, 9, 9) of the cells `index`, upsampled (x8, convex) at pts, sigmoid."""
    w0, b0, w2, b2, w4, b4, w6, b6 = params
    a = F.relu(F.conv2d(x5, w0, b0, padding=1))
    a = F.relu(F.conv2d(a, w2, b2, padding=1))
    a = F.relu(F.conv2d(a, w4, b4, padding=1))
    wl = F.conv2d(a, w6, b6).reshape(a.shape[0], 81).mean(dim=1)
    wlow = torch.zeros(hf * wf, device=wl.device).index_put((index,), wl)
    X, Y = pts[:, 0].long() + crop[1], pts[:, 1].long() + crop[0]
    hc, wc, lane = Y >> 3, X >> 3, (Y & 7) * 8 + (X & 7)
    k = torch.arange(9, device=pts.device)
    s = torch.softmax(mask[(hc * wf + wc)[:, None], k[None] * 64 + lane[:, None]], dim=1)
    ny, nx = hc[:, None] + k[None] // 3 - 1, wc[:, None] + k[None] % 3 - 1
    inside = (ny >= 0) & (ny < hf) & (nx >= 0) & (nx < wf)
    v = torch.where(inside, 8 * wlow[torch.where(inside, ny * wf + nx, torch.zeros_like(ny))], torch.zeros((), device=wl.device))
    return torch.sigmoid((s * v).sum(dim=1) / 8)


def _round(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[500, 2048])
    ap.add_argument("--size", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="file the lines are written to (profiles/wh_train_bench.txt)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the training benchmark needs the MI355X: nothing is measured without it"
    H, W = args.size
    c = Config()
    c.of_class, c.raft_type, c.class_params = RAFTWrapper, "weighted", Config()
    c.class_params.small = c.class_params.mixed_precision = c.class_params.alternate_corr = False
    c.class_params.weight_head_structure = [(128, 3)] * 3
    c.model, c.iters, c.padding_mode = synth.make_state_dict(seed=0), 4, "RAFT"
    prov = RAFTWrapper(c)
    template = synth.make_template(H, W)
    prov.compute_flow(template, synth.make_frame(template, 3), mode="flow", skip_weights=True)
    plan, crop = prov._wh_flow
    params = list(prov.weight_head_parameters().values())
    lines = [f"forward + backward of sum(g * weights_at(pts, do_sigmoid=True)) into the eight head parameters on a {H} x {W} flow "
             f"(precision {prov.precision}); {args.rounds} alternating rounds of {args.reps} calls each after one warm-up round, "
             "ms per call: median (min - max)"]
    for n in args.n:
        idx = np.unique(np.minimum(np.round(H * W * presets.sobol_points(n)).astype(np.int64), H * W - 1))
        pts = torch.from_numpy(np.stack([idx % W, idx // W], 1).astype(np.float32)).cuda()
        g = torch.randn(pts.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        grads = {}

        def hip():
            for p in params:
                p.grad = None
            (prov.weights_at(pts, do_sigmoid=True) * g).sum().backward()
            grads["hip"] = [p.grad for p in params]
        hip()
        state_index = plan._wh_train["dyn"][plan._wh_train["dyn"] >= 0].long()
        n_win = int(state_index.numel())
        x5 = torch.cat([plan.corr.t[state_index, :324].reshape(-1, 81, 4).permute(0, 2, 1).reshape(-1, 4, 9, 9),
                        plan.wmean[state_index].reshape(-1, 1, 1, 1).expand(-1, 1, 9, 9)], dim=1).contiguous()
        mask = plan.mask.t

        def eager():
            for p in params:
                p.grad = None
            (torch_weights_at(x5, params, state_index, mask, pts, plan.hf, plan.wf, crop) * g).sum().backward()
            grads["torch"] = [p.grad for p in params]
        sides = [("hip", hip), ("torch", eager)]
        t = {k: [] for k, _ in sides}
        for r in range(args.rounds + 1):
            for label, fn in sides:
                ms = _round(fn, args.reps)
                if r > 0:                            # (round 0 warms both up)
                    t[label].append(ms)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        agree = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(grads["hip"], grads["torch"]))
        lines.append(f"N={pts.shape[0]:5d} ({n_win} windows) | HIP weights_at fwd + bwd {med['hip']:8.2f} ms ({min(t['hip']):.2f} - "
                     f"{max(t['hip']):.2f}) | float32 torch head + autograd {med['torch']:8.2f} ms ({min(t['torch']):.2f} - "
                     f"{max(t['torch']):.2f}) | torch / HIP = {med['torch'] / med['hip']:.2f} | largest relative gradient difference "
                     f"{agree:.1e}")
        print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
