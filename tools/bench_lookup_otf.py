"""Micro-benchmark of the volume-free lookup (woft_corr_lookup_otf) at 1080p feature size, smooth random flow.
BAND=1: the correlation band instead -- its build, the band lookup and the fallback launch (the volume-free lookup on the miss
flags), isolated, on the smooth field (residual flow 0.3 cells), and on fields scattered by +-3 px and +-8 px per pixel, with the
blocks that missed; the plain volume-free lookup on the same field beside them."""
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from woft_amd import ops
from tools.bench_conv import bench


def main():
    hf, wf, c = 135, 240, 256
    P = hf * wf
    flow = float(os.environ.get("FLOW", "3.0"))
    mk = lambda n: torch.randn(n, c, device="cuda") * 0.3

    def split(t):
        o = torch.zeros(t.shape[0], 2 * c, dtype=torch.bfloat16, device="cuda")
        ops.split_bf16_lines(t, o)
        return o
    f1s = split(mk(P))
    f2s, dims = [], []
    h, w = hf, wf
    for _ in range(4):
        f2s.append(split(mk(h * w)))
        dims.append((h, w))
        h, w = h // 2, w // 2
    idx = torch.arange(P, device="cuda")
    base = torch.stack([idx % wf, idx // wf], 1).float()
    # smooth flow: a global shift + small noise (SMOOTH=0: independent per pixel)
    noise = (torch.rand(P, 2, device="cuda") * 2 - 1) * (flow if os.environ.get("SMOOTH", "1") == "0" else 0.3)
    coords = (base + flow + noise).contiguous()
    out = torch.zeros(P, 352, device="cuda")
    if os.environ.get("BAND", "0") == "1":
        return band(f1s, f2s, dims, hf, wf, c, base, out)
    lp = ops.make_lookup_otf_params(f1s, f2s, dims, hf, wf, c, coords, out, 4, 3)
    lp.ablate = int(os.environ.get("OTF_ABL", "0"))     # developer instances (csrc/lookup_otf.hip: 1, 2, 3, 8, 15, 16 = phase stamps, 64 = stamps in one chunk)
    ms = bench(lambda: ops.run_lookup_otf(lp), reps=20)
    print(f"volume-free lookup {hf}x{wf}, flow {flow}, ablate {lp.ablate}: {ms * 1e3:8.1f} us")
    import numpy as np
    if lp.ablate in (16, 64):
        torch.cuda.synchronize()
        rows = out.view(hf, wf, 352)[::8, ::8, 324:348].contiguous().view(torch.int32).cpu().numpy().astype(np.int64).reshape(-1, 24)
    if lp.ablate == 16:     # per-workgroup timeline (thread 0): start | A fragments + all-level set-up | per level: windows cleared, chunks, next level primed + samples written
        n = int(np.median((rows != 0).sum(axis=1)))
        rows = rows[(rows != 0).sum(axis=1) == n]
        d = np.diff(rows[:, :n], axis=1) & 0xffffffff
        print(f"  start -> set-up barrier (centres, origins / boxes of all levels, A fragments requested) {int(np.median(d[:, 0]))}")
        for l in range((n - 2) // 3):
            print(f"  level {l}: {'box + stream primed + ' if l == 0 else ''}windows cleared {int(np.median(d[:, 1 + 3 * l]))}, chunks {int(np.median(d[:, 2 + 3 * l]))}, "
                  f"next level primed + samples written {int(np.median(d[:, 3 + 3 * l]))}")
        print(f"  workgroup total (median cycles): {int(np.median((rows[:, n - 1] - rows[:, 0]) & 0xffffffff))}")
    if lp.ablate == 64:     # one chunk (level 0, second chunk), per two-K-step group: [top, stream landed, barrier, first fragments, reads + MFMAs (+ DMA issue) done] ... drop
        rows = rows[rows[:, 20] != 0]
        d = np.diff(rows[:, :21], axis=1) & 0xffffffff
        names = ["wait stream", "barrier", "to first fragments", "reads + MFMAs + DMA issue", "to next group / drop"]
        for g in range(4):
            print(f"  group {g}: " + ", ".join(f"{n} {int(np.median(d[:, 5 * g + k]))}" for k, n in enumerate(names)))
        print(f"  chunk total (median cycles): {int(np.median((rows[:, 20] - rows[:, 0]) & 0xffffffff))}  ({len(rows)} workgroups)")


def band(f1s, f2s, dims, hf, wf, c, base, out):
    P = hf * wf
    rows = ops.band_geometry(4, 4)[3]
    buf = torch.zeros(P * rows * ops.BAND_LD, device="cuda")
    miss, count = torch.zeros(P, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda: torch.rand(P, 2, device="cuda", generator=g) * 2 - 1
    fields = [("smooth 0.3 cells", base + 0.3 * rnd()), ("scattered +-3 px", base + 3.0 / 8 * rnd()),
              ("scattered +-8 px", base + 8.0 / 8 * rnd()), ("scattered +-32 px", base + 32.0 / 8 * rnd())]
    first = True
    for name, coords in fields:
        coords = coords.contiguous()
        lp = ops.make_lookup_otf_params(f1s, f2s, dims, hf, wf, c, coords, out, 4, 3)
        bp = ops.make_lookup_band_params(lp, buf, miss, count)
        fb = ops.copy_params(lp)
        fb.need = miss.data_ptr()
        if first:
            print(f"band build {hf}x{wf} ({buf.numel() * 4 / 2**20:.0f} MiB): {bench(lambda: ops.run_band_build(bp), reps=20) * 1e3:8.1f} us")
            first = False
        count.zero_()
        ops.run_lookup_band(bp)
        n_miss = int(count.item())
        t_band = bench(lambda: ops.run_lookup_band(bp), reps=20)
        t_fb = bench(lambda: ops.run_lookup_otf(fb), reps=20)
        t_both = bench(lambda: (ops.run_lookup_band(bp), ops.run_lookup_otf(fb)), reps=20)
        t_otf = bench(lambda: ops.run_lookup_otf(lp), reps=20)
        print(f"{name:18s}: missed blocks {n_miss:4d} of {((hf + 7) // 8) * ((wf + 7) // 8)} | band lookup {t_band * 1e3:7.1f} us, fallback "
              f"{t_fb * 1e3:7.1f} us, both {t_both * 1e3:7.1f} us | volume-free lookup {t_otf * 1e3:7.1f} us")


if __name__ == "__main__":
    main()
