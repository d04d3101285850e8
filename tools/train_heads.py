"""Train one of the two heads of a frozen RAFT on synthetic-homography pairs (woft_amd.hsynth.HSynth): the loop the README shows,
as a command.  Not a trainer framework: one process, one device, batch size one, Adam, no validation, no schedule.

  --head mask    provider.visibility_map() against the pair's dense visibility label:
                 binary_cross_entropy_with_logits(logits[valid], visible[valid])          (raft_type 'weighted_masked')
  --head weight  the reference's own objective (optical_flow/training_configs/*.py): 500 in-frame pixels, their flow,
                 provider.weights_at(pts, do_sigmoid=True), find_homography_nonhomogeneous_QR, and the loss
                 torch_reproj_errors(H_gt, H, pts) clamped at the configs' max_loss       (raft_type 'weighted')

Images: files given on the command line (.npy arrays of (H, W, 3) uint8 BGR; this project reads no image format), cropped to a
multiple of 8, or --textures N synth.make_template textures of --size.  --backgrounds a.npy ... puts one of those images behind the
warped plane, --blur / --noise / --saturation / --hue / --contrast LO HI draw the parameters of woft_amd.hsynth.augment for the
second frame from those ranges and --augment-src blurs and noises the first frame too (HSynth's keywords; all off by default).
--weights synthetic uses the seeded synthetic checkpoint
(with it the numbers mean nothing beyond "the loop runs"); --weights PATH a torch.load-able state dict with the reference's key
set.  Prints the loss of every step, ends with sync_*_head() and a torch.save of the head's parameters to --out.
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import torch.nn.functional as F

from woft_amd import homography as L
from woft_amd import synth
from woft_amd.config import Config
from woft_amd.flow_provider import RAFTWrapper
from woft_amd.hsynth import HSynth

MASK_STRUCTURE = [(128, 3), (128, 3)]          # the shipped 'weighted_masked' head
N_POINTS, MAX_LOSS = 500, 100.0                # the training configs' subsample and max_loss


def make_provider(head, weights, iters, structure=MASK_STRUCTURE):
    masked = head == "mask"
    c = Config()
    c.of_class, c.raft_type, c.class_params = RAFTWrapper, ("weighted_masked" if masked else "weighted"), Config()
    c.class_params.small = c.class_params.mixed_precision = c.class_params.alternate_corr = False
    c.class_params.weight_head_structure = [(128, 3)] * 3
    c.class_params.mask_estimation = masked
    c.class_params.mask_head_structure = structure if masked else None
    if weights == "synthetic":
        c.model = synth.make_state_dict(seed=0, mask_head_structure=structure if masked else None)
    else:
        c.model = torch.load(weights, map_location="cpu")
    c.iters, c.padding_mode, c.weights_postprocessing_fn = iters, "nopad", None
    return RAFTWrapper(c)


def mask_loss(provider, s):
    provider.compute_flow(s.src, s.dst, mode="flow")
    logits = provider.visibility_map()
    return F.binary_cross_entropy_with_logits(logits[s.valid], s.visible[s.valid])


def weight_loss(provider, s, rs, n_points=N_POINTS, max_loss=MAX_LOSS):
    """500 template pixels that the ground truth keeps inside the frame (all of them when fewer), the network's flow at them, the
    head's weights there, the weighted fit, the re-projection error against H_gt."""
    flow = provider.compute_flow(s.src, s.dst, mode="flow", skip_weights=True)[0]
    h, w = s.visible.shape
    gt = s.flow_gt
    ys, xs = torch.meshgrid(torch.arange(h, device=gt.device), torch.arange(w, device=gt.device), indexing="ij")
    px, py = xs + gt[0], ys + gt[1]
    inside = torch.nonzero(((px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)).reshape(-1)).reshape(-1)
    if inside.numel() < 4:
        return None
    pick = torch.from_numpy(np.sort(rs.permutation(inside.numel())[:n_points])).to(inside.device)
    idx = inside[pick]
    pts = torch.stack([idx % w, idx // w], 1).float()
    dst = pts + flow.reshape(2, -1)[:, idx].t()
    wts = provider.weights_at(pts, do_sigmoid=True)
    H = L.find_homography_nonhomogeneous_QR(pts[None], dst[None], wts[None])
    H_gt = torch.from_numpy(s.H_gt).float().to(pts.device)[None]
    err = L.torch_reproj_errors(H_gt, H, pts.t()[None])
    return torch.clamp(err, max=max_loss).mean()


def load_npy(p):
    a = np.load(p)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise SystemExit(f"{p}: an (H, W, 3) uint8 array is expected, got {a.dtype} {a.shape}")
    return a


def load_images(paths, n_textures, size):
    if paths:
        out = []
        for p in paths:
            a = load_npy(p)
            out.append(np.ascontiguousarray(a[:a.shape[0] // 8 * 8, :a.shape[1] // 8 * 8]))
        return out
    return [synth.make_template(size[0], size[1], seq_id=k) for k in range(n_textures)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("images", nargs="*", help=".npy files of (H, W, 3) uint8 BGR images (default: synthetic textures)")
    ap.add_argument("--head", choices=["mask", "weight"], required=True)
    ap.add_argument("--weights", default="synthetic", help="'synthetic' or the path of a state dict")
    ap.add_argument("--size", type=int, nargs=2, default=[256, 320], help="height and width of the synthetic textures")
    ap.add_argument("--textures", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--iters", type=int, default=12, help="RAFT refinement iterations")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="where the head's trained parameters are saved (default <head>_head.pt)")
    ap.add_argument("--backgrounds", nargs="+", default=[], metavar="NPY", help=".npy (H, W, 3) uint8 images put behind the plane")
    ap.add_argument("--blur", type=float, nargs=2, default=[0.0, 0.0], metavar=("LO", "HI"), help="blur sigma range, pixels")
    ap.add_argument("--noise", type=float, nargs=2, default=[0.0, 0.0], metavar=("LO", "HI"), help="noise sigma range, grey levels")
    ap.add_argument("--saturation", type=float, nargs=2, default=[1.0, 1.0], metavar=("LO", "HI"))
    ap.add_argument("--hue", type=float, nargs=2, default=[0.0, 0.0], metavar=("LO", "HI"), help="hue rotation range, radians")
    ap.add_argument("--contrast", type=float, nargs=2, default=[1.0, 1.0], metavar=("LO", "HI"))
    ap.add_argument("--augment-src", action="store_true", help="blur and noise the first frame too")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "training runs on the MI355X: there is no CPU path"
    if args.size[0] % 8 or args.size[1] % 8:
        raise SystemExit("--size: multiples of 8 are expected (the training configs' 'nopad' contract)")
    provider = make_provider(args.head, args.weights, args.iters)
    ds = HSynth(load_images(args.images, args.textures, args.size), seed=args.seed,
                n_occluders=(0, 2) if args.head == "mask" else (0, 1),
                backgrounds=[np.ascontiguousarray(load_npy(p)) for p in args.backgrounds] or None, blur_sigma=args.blur,
                noise_sigma=args.noise, saturation=args.saturation, hue=args.hue, contrast=args.contrast,
                augment_src=args.augment_src)
    params = provider.mask_head_parameters() if args.head == "mask" else provider.weight_head_parameters()
    opt = torch.optim.Adam(list(params.values()), lr=args.lr)
    rs = np.random.RandomState([args.seed, 0x7EAD])
    for step in range(args.steps):
        s = ds.sample(step % len(ds), epoch=step // len(ds))
        loss = mask_loss(provider, s) if args.head == "mask" else weight_loss(provider, s, rs)
        if loss is None or not bool(torch.isfinite(loss)):
            print(f"step {step:5d}  skipped (no usable pixels or a failed fit)", flush=True)
            continue
        opt.zero_grad()
        loss.backward()
        opt.step()
        print(f"step {step:5d}  loss {float(loss.detach()):.6f}", flush=True)
    (provider.sync_mask_head if args.head == "mask" else provider.sync_weight_head)()
    out = args.out or f"{args.head}_head.pt"
    torch.save({k: v.detach().cpu() for k, v in params.items()}, out)
    print(f"saved {len(params)} tensors to {out}", flush=True)


if __name__ == "__main__":
    main()
