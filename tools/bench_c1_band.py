"""Micro-benchmark of an iteration's lookup + convc1 (+ convf1) at 1080p feature size, in isolation: the three launches as they
were -- band lookup, fallback (the volume-free lookup on the miss flags), woft_conv2d_pair(convc1, convf1) -- against the fused
form -- band lookup with the samples deferred, fallback, woft_conv1x1_band.  HIP events, median of 20 after a warm-up, on the
fields of `BAND=1 tools/bench_lookup_otf.py`: smooth (residual flow 0.3 cells), scattered by +-3 px and +-8 px per pixel, and
+-32 px, where every block misses.  --precision bf16x3 | bf16 | fp16."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from woft_amd import _lib, ops
from tools.bench_conv import bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    hf, wf, c = 135, 240, 256
    P = hf * wf
    terms = 1 if a.precision == "bf16" else 3
    mk = lambda n: torch.randn(n, c, device="cuda") * 0.3

    def split(t):
        if terms == 3:
            o = torch.zeros(t.shape[0], 2 * c, dtype=torch.bfloat16, device="cuda")
            ops.split_bf16_lines(t, o)
        else:
            o = torch.zeros(t.shape[0], c, dtype=torch.bfloat16, device="cuda")
            ops.split_bf16(t, o, None)
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
    g = torch.Generator().manual_seed(2)
    pc1 = ops.pack_conv(torch.randn(256, 324, 1, 1, generator=g) * 0.08, torch.randn(256, generator=g) * 0.1)
    pcf = ops.pack_conv(torch.randn(128, 2, 7, 7, generator=g) * 0.1, torch.randn(128, generator=g) * 0.1, flat_cs=4)
    look, flow4 = ops.new_act(1, hf, wf, 324, cs=352, zero=True), ops.new_act(1, hf, wf, 4, zero=True)
    outs = {k: (ops.new_act(1, hf, wf, 256, zero=True), ops.new_act(1, hf, wf, 128, zero=True)) for k in ("old", "new")}
    cp = lambda x, pc, out: ops.conv_params(x, pc, out, epi=_lib.EPI_RELU, precision=a.precision)
    c1 = {k: cp(look, pc1, o[0]) for k, o in outs.items()}
    f1 = {k: cp(flow4, pcf, o[1]) for k, o in outs.items()}
    rows = ops.band_geometry(4, 4)[3]
    buf = torch.zeros(P * rows * ops.BAND_LD, device="cuda")
    miss, count = torch.zeros(P, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    gg = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda: torch.rand(P, 2, device="cuda", generator=gg) * 2 - 1
    fields = [("smooth 0.3 cells", base + 0.3 * rnd()), ("scattered +-3 px", base + 3.0 / 8 * rnd()),
              ("scattered +-8 px", base + 8.0 / 8 * rnd()), ("scattered +-32 px", base + 32.0 / 8 * rnd())]
    print(f"lookup + convc1 + convf1 at {hf}x{wf}, {a.precision} (band terms {terms}); us, median of 20")
    built = False
    for name, coords in fields:
        coords = coords.contiguous()
        flow4.t[:, :2] = coords - base
        lp = ops.make_lookup_otf_params(f1s, f2s, dims, hf, wf, c, coords, look.t, 4, terms)
        bp = ops.make_lookup_band_params(lp, buf, miss, count)
        bd = ops.make_lookup_band_params(lp, buf, miss, count)
        bd.defer_samples = 1
        fb = ops.copy_params(lp)
        fb.need = miss.data_ptr()
        if not built:
            ops.run_band_build(bp)
            built = True
        count.zero_()
        ops.run_lookup_band(bp)
        n_miss = int(count.item())
        old = lambda: (ops.run_lookup_band(bp), ops.run_lookup_otf(fb), ops.run_conv_pair(c1["old"], f1["old"]))
        new = lambda: (ops.run_lookup_band(bd), ops.run_lookup_otf(fb), ops.run_conv1x1_band(c1["new"], f1["new"], bd))
        look.t.zero_()
        old()
        look.t.fill_(float("nan"))                          # (a sample the fused form took from the buffer of a hit block would show)
        look.t[:, 324:] = 0
        new()
        torch.cuda.synchronize()
        same = all(torch.equal(x.t, y.t) for x, y in zip(outs["old"], outs["new"]))
        t = {"band lookup": bench(lambda: ops.run_lookup_band(bp), reps=20), "deferred": bench(lambda: ops.run_lookup_band(bd), reps=20),
             "fallback": bench(lambda: ops.run_lookup_otf(fb), reps=20),
             "conv pair": bench(lambda: ops.run_conv_pair(c1["old"], f1["old"]), reps=20),
             "fused": bench(lambda: ops.run_conv1x1_band(c1["new"], f1["new"], bd), reps=20),
             "old three": bench(old, reps=20), "new three": bench(new, reps=20)}
        print(f"{name:18s}: missed blocks {n_miss:4d} of {((hf + 7) // 8) * ((wf + 7) // 8)} | "
              + ", ".join(f"{k} {v * 1e3:6.1f}" for k, v in t.items())
              + f" | saved {(t['old three'] - t['new three']) * 1e3:6.1f} | outputs {'identical' if same else 'DIFFER'}")


if __name__ == "__main__":
    main()
