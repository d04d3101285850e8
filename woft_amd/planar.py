"""The device planar stage every tracker shares ("The planar stage"): after a tracker's own selection launch,
ONE fit-and-judge step, ONE pinned read of ONE result block and ONE pure decoder, for K >= 1 targets.  The block, as planes of
32-bit words (K = 1 is the same layout, not a second one; `hist` only for the chained multi-target tracker):

    H (K, 9) f32 | frac (K) f32 | status (K) i32 | count (2, K) i32 = selected, kept | hist (K, ops.CHAIN_HIST) i32
"""
import time
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch

from . import ops


class _Fit(SimpleNamespace):
    """Result of one solve: H (3x3 float64, cur -> src) and, for the global stage, the re-detection verdict."""


def block_words(K, with_hist):
    return K * (13 + (ops.CHAIN_HIST if with_hist else 0))


def block_views(f32, i32, K, with_hist):
    """Named views of a block's words, given as float32 and as int32 (torch tensors or numpy arrays): the only index arithmetic."""
    return SimpleNamespace(H=f32[:9 * K].reshape(K, 9), frac=f32[9 * K:10 * K], status=i32[10 * K:11 * K],
                           count=i32[11 * K:13 * K].reshape(2, K), selected=i32[11 * K:12 * K], kept=i32[12 * K:13 * K],
                           hist=i32[13 * K:].reshape(K, ops.CHAIN_HIST) if with_hist else None)


class ResultBlock:
    """The zero-filled device block of K targets with its named views; on a GPU also the pinned host mirror and read()'s event."""

    def __init__(self, K, device, with_hist=False):
        self.dev = torch.zeros(block_words(K, with_hist), dtype=torch.float32, device=device)
        vars(self).update(vars(block_views(self.dev, self.dev.view(torch.int32), K, with_hist)))
        self.host, self.event = ((torch.empty(self.dev.numel(), dtype=torch.float32).pin_memory(), torch.cuda.Event())
                                 if self.dev.is_cuda else (None, None))

    def read(self):
        """The stage's single device->host read: into the pinned mirror (no staging copy, no allocation), then wait for it ->
        the seconds this thread was blocked (the caller adds them to its `host_wait_s`)."""
        self.host.copy_(self.dev, non_blocking=True)
        self.event.record()
        t0 = time.perf_counter()
        self.event.synchronize()
        return time.perf_counter() - t0


def decode(block_f32, K, spec, with_hist):
    """The host mirror of a block (numpy float32) -> per target (fit | None, selected, kept, hist int64 | None).  Status 1 (too few
    points for the estimator) is no fit; any other status a _Fit with the block's H as a float64 copy, NaN included.  The verdict is
    the spec's `const_verdict` (a re-detection test that is `return True` / `return False`: the reference's ablations) or
    frac > min_frac in float32, as torch compares a float32 mean with a Python float."""
    v = block_views(block_f32, block_f32.view(np.int32), K, with_hist)
    const, out = spec.get("const_verdict"), []
    for t in range(K):
        fit = None
        if int(v.status[t]) != 1:
            verdict = const if const is not None else bool(np.float32(v.frac[t]) > np.float32(spec["min_frac"]))
            fit = _Fit(H=v.H[t].astype(np.float64).reshape(3, 3), success=bool(verdict))        # (astype: a copy)
        out.append((fit, int(v.selected[t]), int(v.kept[t]), v.hist[t].astype(np.int64) if with_hist else None))
    return out


class PlanarBuffers:
    """What one planar stage of K targets on an n_grid-pixel flow writes: the selection's scratch `ws`, the selected correspondences
    `pa`, `pb`, `w` (cap per target), the estimator's scratch `fit_ws` and the result block.  batched: (K, cap, ...) buffers for the
    K-target entry points; else (cap, ...) ones for the single-target entry points (K = 1)."""

    def __init__(self, spec, K, n_grid, cap, device, batched, with_hist=False):
        new = lambda *s: torch.empty(((K,) if batched else ()) + s, dtype=torch.float32, device=device)
        self.cap, self.batched = cap, batched
        self.ws = ops.tc_select_multi_ws(n_grid, K) if batched else ops.tc_select_ws(n_grid)
        self.pa, self.pb, self.w = new(cap, 2), new(cap, 2), new(cap)
        self.block = blk = ResultBlock(K, device, with_hist)
        R, T = spec.get("ransac"), spec.get("trs")
        self.fit_ws = (ops.trs_ws(cap, T["max_iters"], device) if T is not None else
                       ops.ransac_ws(cap, R["max_iters"], device) if R is not None else
                       ops.hfit_ws(device) if (not batched and cap > ops.HFIT_SINGLE_MAX) else None)      # (the streaming fit's)
        # per target (pa, pb, H, status, selected), as the single-element estimators (RANSAC, TRS) take them
        self.targets = ([(self.pa[t], self.pb[t], blk.H[t], blk.status[t:t + 1], blk.selected[t:t + 1]) for t in range(K)]
                        if batched else [(self.pa, self.pb, blk.H, blk.status, blk.selected)])


def fit_and_judge(spec, b, weighted):
    """On the selection's output in `b`: RANSAC or TRS once per target on that target's slices (status 1 / 2: too few points / no
    model, H all NaN), else the least-squares / IRLS fit; then the inlier test.  Every result lands in b.block."""
    blk, w = b.block, (b.w if weighted else None)
    R, T = spec.get("ransac"), spec.get("trs")
    if R is not None or T is not None:
        fn, P = (ops.ransac, R) if R is not None else (ops.trs, T)
        for pa, pb, H, status, selected in b.targets:
            fn(pa, pb, H, status, count=selected, max_iters=P["max_iters"], thr=P["thr"], conf=P["conf"], ws=b.fit_ws)
    else:
        irls = dict(reweight=spec["reweight"], huber_k=spec["huber_k"], n_irls=spec["n_irls"])
        if b.batched:
            ops.hfit_batched(b.pa, b.pb, w, blk.H, blk.status, counts=blk.selected, **irls)
        else:
            ops.hfit(b.pa, b.pb, w, blk.H, blk.status, count=blk.selected, ws=b.fit_ws, **irls)
    (ops.inlier_frac_batched if b.batched else ops.inlier_frac)(b.pa, b.pb, blk.H, blk.frac, spec["thr"], blk.selected)


class BoundedCache(OrderedDict):
    """Keyed buffers, at most `limit` of them: one more drops the least recently used (limit 1: a new key replaces the old one)."""

    def __init__(self, limit=1):
        super().__init__()
        self.limit = limit

    def lookup(self, key, make):
        if key in self:
            self.move_to_end(key)
            return self[key]
        return self.put(key, make())

    def put(self, key, value):
        self[key] = value
        while len(self) > self.limit:
            self.popitem(last=False)
        return value
