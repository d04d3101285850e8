"""Forward + backward of the differentiable weighted least-squares fit (find_homography_nonhomogeneous_QR with a weight that
requires grad: woft_hfit / woft_hfit_batched forward, woft_hfit_batched_bwd backward) against what a user had before it: the
same loss through a plain float32 torch restatement of least_squares_H.py:142-210 on the device (Hartley normalisation, the
(2N x 8) system, torch.linalg.qr, triangular solve), differentiated by torch autograd.  The restatement lives here, not in the
product.  N = 500, B = 1, 8, 64 by default; loss = torch_reproj_errors(GT_H, H, pts).mean() as the training configs form it;
one process, alternating rounds, HIP events around each round's calls.  The lines go to --out
(profiles/hfit_backward_bench.txt)."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from woft_amd import homography as Hm


def _normalize(p, eps=1e-8):
    mean = p.mean(dim=1, keepdim=True)
    scale = (2.0 ** 0.5) / ((p - mean).norm(dim=-1).mean(dim=-1) + eps)
    one, zero = torch.ones_like(scale), torch.zeros_like(scale)
    T = torch.stack([scale, zero, -scale * mean[:, 0, 0], zero, scale, -scale * mean[:, 0, 1], zero, zero, one], dim=-1).view(-1, 3, 3)
    return scale[:, None, None] * (p - mean), T


def torch_fit(points1, points2, weights):
    """The reference's estimator in plain float32 torch ops (what autograd differentiates through torch.linalg.qr)."""
    p1, T1 = _normalize(points1)
    p2, T2 = _normalize(points2)
    x1, y1, x2, y2 = p1[..., 0:1], p1[..., 1:2], p2[..., 0:1], p2[..., 1:2]
    one, zero = torch.ones_like(x1), torch.zeros_like(x1)
    ax = torch.cat([zero, zero, zero, -x1, -y1, -one, y2 * x1, y2 * y1], dim=-1)
    ay = torch.cat([x1, y1, one, zero, zero, zero, -x2 * x1, -x2 * y1], dim=-1)
    B, N = x1.shape[:2]
    A = torch.stack([ax, ay], dim=2).reshape(B, 2 * N, 8)
    b = torch.stack([-y2, x2], dim=2).reshape(B, 2 * N, 1)
    w = weights[:, :, None].repeat(1, 1, 2).reshape(B, 2 * N, 1)
    A, b = w * A, w * b
    Q, R = torch.linalg.qr(A)
    sol = torch.linalg.solve_triangular(R, Q.transpose(-1, -2) @ b, upper=True)
    H = torch.cat([sol, torch.ones_like(sol[:, :1])], dim=1).view(-1, 3, 3)
    H = torch.linalg.inv(T2) @ (H @ T1)
    return H / (H[..., -1:, -1:] + 1e-8)


def _round(fn, reps):
    """microseconds per call of `reps` back-to-back calls (HIP events around the lot, ending in a synchronise)."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="file the lines are written to (profiles/hfit_backward_bench.txt)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the backward benchmark needs the MI355X: nothing is measured without it"
    n = args.n
    lines = [f"forward + backward of loss = torch_reproj_errors(GT_H, fit(a, b, w), pts).mean() with respect to w, a, b; N = {n}; "
             f"{args.rounds} alternating rounds of {args.reps} calls each after one warm-up round, us per call: median (min - max)"]
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in args.batch:
        a = torch.stack([torch.rand(B, n, device="cuda", generator=g) * 1700 + 100,
                         torch.rand(B, n, device="cuda", generator=g) * 920 + 80], -1).contiguous()
        b = (a * 1.01 + torch.tensor([3.0, -2.0], device="cuda") + torch.randn(B, n, 2, device="cuda", generator=g) * 0.5).contiguous()
        w = (torch.rand(B, n, device="cuda", generator=g) * 0.9 + 0.05).contiguous()
        gt = torch.tensor([[1.012, 0.001, 2.5], [-0.001, 1.008, -2.2], [0.0, 0.0, 1.0]], device="cuda").expand(B, 3, 3).contiguous()
        pts = (torch.rand(B, 2, 16, device="cuda", generator=g) * 16).contiguous()
        grads = {}

        def step(fit, label):
            ta, tb, tw = a.clone().requires_grad_(), b.clone().requires_grad_(), w.clone().requires_grad_()
            loss = Hm.torch_reproj_errors(gt, fit(ta, tb, tw), pts).mean()
            loss.backward()
            grads[label] = (ta.grad, tb.grad, tw.grad)
        sides = [("hip", lambda: step(Hm.find_homography_nonhomogeneous_QR, "hip")), ("torch", lambda: step(torch_fit, "torch"))]
        t = {k: [] for k, _ in sides}
        try:
            for r in range(args.rounds + 1):
                for label, fn in sides:
                    us = _round(fn, args.reps)
                    if r > 0:                        # (round 0 warms both up)
                        t[label].append(us)
        except RuntimeError as err:                  # (e.g. no device QR in this torch build: say so, claim nothing)
            lines.append(f"B={B:3d} | not measured: {type(err).__name__}: {str(err).splitlines()[0][:160]}")
            print(lines[-1], flush=True)
            continue
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        agree = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(grads["hip"], grads["torch"]))
        lines.append(f"B={B:3d} | HIP fit + HIP backward {med['hip']:9.1f} us ({min(t['hip']):.1f} - {max(t['hip']):.1f})"
                     f" | float32 torch QR + autograd {med['torch']:9.1f} us ({min(t['torch']):.1f} - {max(t['torch']):.1f})"
                     f" | torch / HIP = {med['torch'] / med['hip']:.2f} | largest relative gradient difference {agree:.1e}")
        print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
