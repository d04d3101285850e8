"""Generate the MaskHead fixtures (tests/golden/mask_*.npz) by running the REFERENCE itself.

Run only where the reference checkout is present (the GPU tests read the fixtures, never the reference):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_mask.py

Uses oracle.gen_golden's stubs and helpers unchanged.  Two fixtures:
  mask_head_128x160_it4.npz     WeightedRAFT(mask_estimation=True) (weighted_raft.py:75-76,295-309,387-422): full model with
                                mask_head_structure [(128, 3), (128, 3)], small model with [(64, 5), 32]; flow, weight logits,
                                the 1/8-resolution mask logits (the MaskHead's own output) and mask_up, + the head's key/shape list
  mask_wrapper_128x160_it4.npz  the reference's RAFTWrapper with raft_type 'weighted_masked' (optical_flow/raft.py:38-42,
                                142-147,170-216): mode 'flow' and 'TC' (nopad), RAFT padding at 125x157, crop at 128x157,
                                numpy_out once (what these return beyond the mask is asserted here, not stored)
"""
import json
import os
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle.gen_golden import GOLD, REF, install_stubs, pair, to_t  # noqa: E402
from woft_amd import synth  # noqa: E402

CASES = {"full": dict(small=False, seed=7, pair_seed=11, structure=[(128, 3), (128, 3)]),
         "small": dict(small=True, seed=9, pair_seed=13, structure=[(64, 5), 32])}
ITERS = 4


def _args(small, structure):
    return SimpleNamespace(small=small, mixed_precision=False, alternate_corr=False, weight_head_structure=[(128, 3)] * 3,
                           mask_estimation=True, mask_head_structure=structure)


@torch.no_grad()
def gen_model():
    from raft_core.weighted_raft import WeightedRAFT
    out = dict(iters=ITERS, names=np.array(sorted(CASES)))
    keys = {}
    for name, c in CASES.items():
        sd = synth.make_state_dict(seed=c["seed"], small=c["small"], weighted=True, mask_head_structure=c["structure"])
        net = WeightedRAFT(_args(c["small"], c["structure"])).eval()
        net.load_state_dict(sd, strict=True)
        keys[name] = {k: list(v.shape) for k, v in net.state_dict().items() if k.startswith("mask_head.")}
        low = []
        hook = net.mask_head.register_forward_hook(lambda m, i, o: low.append(o.detach().clone()))
        a, b = pair(128, 160, seed=c["pair_seed"])
        flow_low, flow_up, _, w_low, w_up, mask_up = net(to_t(a), to_t(b), iters=ITERS, test_mode=True)
        hook.remove()
        assert len(low) == 1 and tuple(mask_up.shape) == (1, 1, 128, 160)
        out.update({f"{name}_img1": a, f"{name}_img2": b, f"{name}_seed": c["seed"], f"{name}_small": int(c["small"]),
                    f"{name}_structure": json.dumps(c["structure"]),
                    f"{name}_flow_up": flow_up.numpy(), f"{name}_w_up": w_up.numpy(),
                    f"{name}_mask_low": low[0].numpy(), f"{name}_mask_up": mask_up.numpy()})
    out["mask_head_keys"] = json.dumps(keys)
    np.savez_compressed(GOLD / "mask_head_128x160_it4.npz", **out)


@torch.no_grad()
def gen_wrapper():
    """The reference's own wrapper, configured from its own config loader (as oracle.gen_golden.gen_wrapper)."""
    from pytracking.utils.config import load_config
    c = CASES["full"]
    fc = load_config(REF / "pytracking/optical_flow/configs/v2_SNOB_large_g05_RAFT.py")
    fc.weights_postprocessing_fn = None
    fc.raft_type = "weighted_masked"
    fc.class_params.mask_estimation = True
    fc.class_params.mask_head_structure = c["structure"]
    sd = synth.make_state_dict(seed=c["seed"], mask_head_structure=c["structure"])
    o = {}
    with tempfile.TemporaryDirectory() as td:
        fc.model = os.path.join(td, "sd.pth")
        torch.save(sd, fc.model)
        fc.iters = ITERS
        flower = fc.of_class(fc)
        a, b = pair(128, 160, seed=c["pair_seed"])
        o["src"], o["dst"], o["w"], o["m"] = flower.compute_flow(a, b, mode="TC", do_sigmoid=True)
        o["flow"], o["w_logit"], o["m_flow"] = flower.compute_flow(a, b, mode="flow", do_sigmoid=False)
        o["np_flow"], o["np_w"], o["np_m"] = flower.compute_flow(a, b, mode="flow", numpy_out=True)
        fc.padding_mode = "RAFT"
        a2, b2 = a[:125, :157].copy(), b[:125, :157].copy()
        o["src_pad"], o["dst_pad"], o["w_pad"], o["m_pad"] = flower.compute_flow(a2, b2, mode="TC", do_sigmoid=True)
        fc.padding_mode = "crop"
        a4, b4 = a[:, :157].copy(), b[:, :157].copy()
        o["src_crop"], o["dst_crop"], o["w_crop"], o["m_crop"] = flower.compute_flow(a4, b4, mode="TC", do_sigmoid=True)
    for k in ("np_flow", "np_w", "np_m"):
        assert isinstance(o[k], np.ndarray), k
    o = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}
    # (the fixture keeps what the mask adds, each once, within the size limit for a committed file; the rest is asserted here:
    #  the source grids are the pixel grid, the mask does not depend on the mode or on numpy_out)
    for s_, shape in (("src", (128, 160)), ("src_pad", (125, 157)), ("src_crop", (128, 152))):
        ys, xs = np.mgrid[:shape[0], :shape[1]]
        assert np.array_equal(o[s_], np.stack([xs.ravel(), ys.ravel()])), s_
    assert np.array_equal(o["m"].reshape(o["m_flow"].shape), o["m_flow"]) and np.array_equal(o["m_flow"], o["np_m"])
    assert np.array_equal(o["flow"], o["np_flow"]) and o["m_crop"].shape == (1, 128 * 152)
    np.savez_compressed(GOLD / "mask_wrapper_128x160_it4.npz", img1=a, img2=b, seed=c["seed"], iters=ITERS,
                        structure=json.dumps(c["structure"]), dst=o["dst"], w=o["w"], m=o["m"], w_logit=o["w_logit"],
                        m_pad=o["m_pad"], m_crop=o["m_crop"])


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    install_stubs()
    gen_model()
    gen_wrapper()
    for p in sorted(GOLD.glob("mask_*.npz")):
        print(f"{p.name:40s} {p.stat().st_size / 1024:9.1f} KB")


if __name__ == "__main__":
    main()
