"""Cost of the MaskHead ('weighted_masked') per flow: microseconds per launch of woft_warp_features and of
the whole mask program (warp -> head layers -> closing 1x1 conv -> convex upsampling of the logits), at 1080p and 4K, timed
with HIP events after warm-up on the engine's own buffers (one flow is run first so that coordinates and features are real).

    python tools/bench_mask_head.py [--reps 50] [--precision bf16x3 fp32] [--structure '[[128, 3], [128, 3]]']
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from woft_amd import ops, synth  # noqa: E402
from woft_amd.engine import RaftEngine  # noqa: E402


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1000.0 * s.elapsed_time(e) / reps


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--precision", nargs="+", default=["bf16x3", "fp32"])
    ap.add_argument("--structure", default="[[128, 3], [128, 3]]")
    a = ap.parse_args()
    st = [tuple(x) if isinstance(x, list) else x for x in json.loads(a.structure)]
    sd = synth.make_state_dict(seed=0, mask_head_structure=st)
    print(f"# MaskHead cost per flow, structure {st}, {a.reps} timed repetitions after 5 warm-up ones (HIP events)")
    print(f"{'res':>6s} {'precision':>9s} {'warp us':>9s} {'layers us':>10s} {'1x1 us':>8s} {'upsample us':>12s} {'program us':>11s}"
          f" {'warp GB/s':>10s} {'layer-1 TFLOP/s':>16s}")
    for name, (H, W) in (("1080p", (1080, 1920)), ("4K", (2160, 3840))):
        for prec in a.precision:
            eng = RaftEngine(sd, precision=prec, corr="otf", mask_head=True)
            plan = eng.plan(H, W)
            img = synth.make_template(H, W, seq_id=0)
            plan.load_image(0, torch.from_numpy(img).cuda(), 0, 0)
            plan.load_image(1, torch.from_numpy(synth.make_frame(img, 2)).cuda(), 0, 0)
            plan.encode_source()
            mout = torch.empty(1, H * W, device="cuda")
            plan.flow(4, (0, 0), H, W, dst=torch.empty(2, H * W, device="cuda"), mout=mout)
            t_warp = timed(lambda: ops.warp_features(plan.f2act[0], plan.coords, plan.mh_warped), a.reps)

            def layers():
                for p in plan.prog_mh:
                    ops.run_conv(p)
            t_layers = timed(layers, a.reps)
            t_full = timed(plan._mask_head, a.reps)
            t_up = timed(lambda: ops.convex_upsample(plan.coords, plan.mh_low, plan.mask.t, plan.hf, plan.wf, (0, 0), H, W,
                                                     wout=mout), a.reps)
            t_1x1 = t_full - t_warp - t_layers
            P, c = plan.P, eng.spec.fdim
            gbs = 2 * P * c * 4 / (t_warp * 1e-6) / 1e9                 # unique reads of fmap2 + writes, bytes / s
            sh = eng.mh_shapes[0]
            tflops = 2 * P * sh[0] * sh[1] * sh[2] * sh[3] / (plan_layer0_us(plan, a.reps) * 1e-6) / 1e12
            print(f"{name:>6s} {prec:>9s} {t_warp:9.1f} {t_layers:10.1f} {t_1x1:8.1f} {t_up:12.1f} {t_full + t_up:11.1f}"
                  f" {gbs:10.0f} {tflops:16.1f}")
            plan = eng = None
            torch.cuda.empty_cache()


def plan_layer0_us(plan, reps):
    return timed(lambda: ops.run_conv(plan.prog_mh[0]), reps)


if __name__ == "__main__":
    main()
