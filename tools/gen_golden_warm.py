"""Generate the warm-start fixture tests/golden/warm_start_128x160_it4.npz by running the REFERENCE itself.

Run only where the reference checkout is present (the tests read the fixture, never the reference):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_warm.py

Uses oracle.gen_golden's stubs and helpers unchanged.  The fixture holds
  * three networks run with a `flow_init` (weighted_raft.py:184,223-224), 128 x 160, 4 iterations: WeightedRAFT full,
    WeightedRAFT small and a 'weighted_masked' WeightedRAFT (mask_estimation=True) -- images (one copy per image pair:
    `<case>_images` names the case that holds them), seeds, flow_init, flow_low, flow_up, w_up (and mask_up);
  * four forward_interpolate cases (raft_core/utils/utils.py:28-56, scipy's griddata): small flow at 16 x 20, large flow at
    16 x 20 (about half the points leave the grid), 17 x 23, and a field with exactly one valid point.  Every case is
    re-seeded until, at every cell, the nearest and the second-nearest landing point differ by more than 1e-9 in squared
    distance: neither scipy's unspecified tie order nor a last-bit rounding difference enters the comparison.
Arrays only.
"""
import json
import os
import sys
from pathlib import Path
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle.gen_golden import GOLD, install_stubs, pair, ref_args, to_t  # noqa: E402
from woft_amd import synth  # noqa: E402

ITERS = 4
MASK_STRUCTURE = [(128, 3), (128, 3)]
NETS = {"full": dict(small=False, seed=7, pair_seed=11, init_seed=101, structure=None),
        "small": dict(small=True, seed=9, pair_seed=13, init_seed=102, structure=None),
        "masked": dict(small=False, seed=7, pair_seed=11, init_seed=103, structure=MASK_STRUCTURE)}
FI_CASES = {"small_16x20": dict(hf=16, wf=20, kind="small", seed=201),
            "large_16x20": dict(hf=16, wf=20, kind="large", seed=202),
            "odd_17x23": dict(hf=17, wf=23, kind="small", seed=203),
            "one_valid_16x20": dict(hf=16, wf=20, kind="one", seed=204)}
MIN_GAP = 1e-9


def make_flow_init(hf, wf, seed):
    """A smooth field of a few 1/8-resolution pixels plus noise, (2, hf, wf) fp32."""
    rs = np.random.RandomState(seed)
    ys, xs = np.mgrid[:hf, :wf]
    u = 1.5 * np.sin(xs / wf * 2.3 + 0.4) + 0.8 * ys / hf - 0.6
    v = -1.2 * np.cos(ys / hf * 1.9) + 0.5 * xs / wf + 0.3
    f = np.stack([u, v]) + rs.normal(0.0, 0.15, (2, hf, wf))
    return f.astype(np.float32)


def make_fi_flow(hf, wf, kind, seed):
    rs = np.random.RandomState(seed)
    if kind == "small":
        return (make_flow_init(hf, wf, seed) + rs.uniform(-0.5, 0.5, (2, hf, wf))).astype(np.float32)
    if kind == "large":         # displacements of the order of the grid: about half of the points land outside
        return np.stack([rs.uniform(-0.75 * wf, 0.75 * wf, (hf, wf)), rs.uniform(-0.75 * hf, 0.75 * hf, (hf, wf))]).astype(np.float32)
    # exactly one valid point: everything is thrown far outside, one point stays
    f = np.stack([rs.uniform(2.0 * wf, 3.0 * wf, (hf, wf)), rs.uniform(-3.0 * hf, -2.0 * hf, (hf, wf))]).astype(np.float32)
    y, x = int(rs.randint(1, hf - 1)), int(rs.randint(1, wf - 1))
    f[:, y, x] = rs.uniform(-0.4, 0.4, 2)
    return f


def gaps(flow):
    """-> (number of valid points, smallest difference between nearest and second-nearest squared distance over the cells)."""
    _, hf, wf = flow.shape
    ys, xs = np.mgrid[:hf, :wf]
    x1 = (xs + flow[0].astype(np.float64)).reshape(-1)
    y1 = (ys + flow[1].astype(np.float64)).reshape(-1)
    valid = (x1 > 0) & (x1 < wf) & (y1 > 0) & (y1 < hf)
    ddx = xs.reshape(-1, 1) - x1[valid][None]
    ddy = ys.reshape(-1, 1) - y1[valid][None]
    d = np.sort(ddx * ddx + ddy * ddy, axis=1)
    return int(valid.sum()), (float((d[:, 1] - d[:, 0]).min()) if d.shape[1] > 1 else float("inf"))


@torch.no_grad()
def gen_nets(out):
    from raft_core.weighted_raft import WeightedRAFT
    for name, c in NETS.items():
        if c["structure"]:
            sd = synth.make_state_dict(seed=c["seed"], small=c["small"], weighted=True, mask_head_structure=c["structure"])
            args = SimpleNamespace(small=c["small"], mixed_precision=False, alternate_corr=False,
                                   weight_head_structure=[(128, 3)] * 3, mask_estimation=True, mask_head_structure=c["structure"])
        else:
            sd = synth.make_state_dict(seed=c["seed"], small=c["small"], weighted=True)
            args = ref_args(c["small"])
        net = WeightedRAFT(args).eval()
        net.load_state_dict(sd, strict=True)
        a, b = pair(128, 160, seed=c["pair_seed"])
        init = make_flow_init(16, 20, c["init_seed"])
        res = net(to_t(a), to_t(b), iters=ITERS, flow_init=torch.from_numpy(init)[None], test_mode=True)
        flow_low, flow_up, w_up = res[0], res[1], res[4]
        shared = next((n for n in out.get("_pairs", {}) if out["_pairs"][n] == c["pair_seed"]), None)
        out.setdefault("_pairs", {})[name] = c["pair_seed"]
        if shared is None:
            out.update({f"{name}_img1": a, f"{name}_img2": b})
        out[f"{name}_images"] = shared or name       # (the case whose img1 / img2 these are: one copy per image pair)
        out.update({f"{name}_seed": c["seed"], f"{name}_pair_seed": c["pair_seed"],
                    f"{name}_init_seed": c["init_seed"], f"{name}_small": int(c["small"]), f"{name}_flow_init": init,
                    f"{name}_flow_low": flow_low.numpy(), f"{name}_flow_up": flow_up.numpy(), f"{name}_w_up": w_up.numpy()})
        if c["structure"]:
            out[f"{name}_mask_up"] = res[5].numpy()
            out[f"{name}_structure"] = json.dumps(c["structure"])
        print(f"{name}: |flow_low - flow_init| mean {float(np.abs(flow_low.numpy()[0] - init).mean()):.3f}")


def gen_fi(out):
    from raft_core.utils.utils import forward_interpolate
    for name, c in FI_CASES.items():
        seed = c["seed"]
        while True:
            flow = make_fi_flow(c["hf"], c["wf"], c["kind"], seed)
            n_valid, gap = gaps(flow)
            want_one = c["kind"] == "one"
            if gap > MIN_GAP and n_valid >= 1 and (n_valid == 1) == want_one:
                break
            seed += 1000
        assert gap > MIN_GAP, (name, gap)
        res = forward_interpolate(torch.from_numpy(flow)).numpy()
        assert res.dtype == np.float32 and res.shape == flow.shape
        out.update({f"fi_{name}_flow": flow, f"fi_{name}_out": res, f"fi_{name}_seed": seed, f"fi_{name}_valid": n_valid})
        print(f"fi {name}: seed {seed}, {n_valid} of {flow[0].size} points valid, smallest gap {gap:.3e}")


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    install_stubs()
    out = dict(iters=ITERS, names=np.array(sorted(NETS)), fi_names=np.array(sorted(FI_CASES)), min_gap=MIN_GAP)
    gen_fi(out)
    gen_nets(out)
    out.pop("_pairs")
    p = GOLD / "warm_start_128x160_it4.npz"
    np.savez_compressed(p, **out)
    print(f"{p.name:40s} {p.stat().st_size / 1024:9.1f} KB")


if __name__ == "__main__":
    main()
