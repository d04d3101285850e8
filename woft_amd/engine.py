"""RAFT / WeightedRAFT inference engine on the HIP kernels (full and small models).

Host-side orchestration only: packs a reference-format state-dict once, plans every buffer and
every kernel-argument struct once per input resolution, then a frame is a fixed sequence of C-ABI
calls on torch's current stream -- no allocation, no host synchronisation inside.

Reference being replaced (paths under /root/reference/pytracking/external/RAFT/raft_core/):
  WeightedRAFT.forward  weighted_raft.py:179-315      RAFT.forward  raft.py:169-262
  BasicEncoder / SmallEncoder  extractor.py:118-267   CorrBlock     corr.py:11-69
  BasicUpdateBlock / SmallUpdateBlock  update.py:99-136   WeightHead  weighted_raft.py:318-384
  MaskHead (opt-in, mask_head=True)  weighted_raft.py:295-309,387-422

Results-identical restructurings: BatchNorm(eval) folded into the cnet convs; the
mask head evaluated only after the last iteration (test_mode consumes only that one,
weighted_raft.py:240-255); pyramid levels built as correlations against 2x2-pooled fmap2
(linearity; the reference's own AlternateCorrBlock does the same, corr.py:77-81); the weight
head's mean-response channel in algebraic form; template-side tensors (fmap1, net, inp) cached
when the caller pins the source image.

Launch programs: lists of Step(kind, arg, tag) replayed by _Plan.run().  A refinement iteration has up to three (first / middle /
merged last) and, with the flow-head gather folded into the next lookup, a second set (_Plan.folded): _Plan._iteration() alone
picks among them.  The heads after the loop (prog_mask, prog_wh, prog_mh) are plain lists of conv parameter structs.

A plan alone knows what its buffers hold (source_owner, target_owner, target_valid, band_valid: _source_changed / _target_changed)
and owns the captured hipGraphs of its flow() (flow(graph=True), FlowKey); callers ask, they keep no copy of either.
"""
import math
import os
from typing import NamedTuple

import torch

from . import _lib, conv_select, flow_region, mh_train, ops, wh_train
from .conv_select import KERNELS, Kernel
from .ops import Act, new_act

EPI = _lib
# InstanceNorm encoders: conv1's output and the downsample branch stay raw for their consumers to normalise (0: materialised)
DEFER_NORM = os.environ.get("WOFT_DEFER_NORM", "1") != "0"
# flow head: the 3x3 -> 2-channel conv folded into the first conv's epilogue + a per-pixel gather (0: two convs, the
# second on the vector ALUs in exact fp32 -- woft_flow_head_update)
FUSE_FLOWHEAD = os.environ.get("WOFT_FUSE_FLOWHEAD", "1") != "0"
# motion encoder: the correlation branch (convc1 -> convc2) and the flow branch (convf1 -> convf2) are independent until
# `conv` joins them (update.py:89-97): first layers in one launch, second layers in one launch (woft_conv2d_pair)
PAIR_BRANCHES = os.environ.get("WOFT_PAIR", "1") != "0"
PYRAMID_ONE_LAUNCH = os.environ.get("WOFT_PYRAMID", "1") != "0"    # target pyramid (pool + split of all levels) in one launch
# the flow-head gather of iteration k runs inside the lookup launch of iteration k + 1 (volume-free lookup; the last
# iteration's as its own launch): one launch fewer per iteration, same operations in the same order (0: always its own launch)
FOLD_GATHER = os.environ.get("WOFT_FOLD_GATHER", "1") != "0"
# correlation band (include/woft_hip.h: woft_lookup_band_params): the correlations of the volume-free lookup
# around the identity are computed once per flow (woft_corr_band_build) and every lookup samples from them
# (woft_corr_lookup_band), the volume-free lookup itself computing the 8 x 8 blocks whose windows left the band.  Bit-identical
# results.  RaftEngine(corr_band=): "auto" = flows of at least BAND_MIN_LOOKUPS lookups, True = every flow the band applies to,
# False = none; WOFT_CORR_BAND=0 switches it off everywhere.
CORR_BAND = os.environ.get("WOFT_CORR_BAND", "1") != "0"
# convc1 samples the band inside its own launch (csrc/conv_1x1_band.hip): on a plan with a valid band an
# unrestricted iteration runs the band lookup with its samples deferred, the fallback, and woft_conv1x1_band in place of
# conv2(convc1, convf1) -- the samples of hit blocks never reach memory.  Bit-identical results.  RaftEngine(fuse_c1=False) or
# WOFT_FUSE_C1=0: the three launches as they were (A/Bs, tests).
FUSE_C1 = os.environ.get("WOFT_FUSE_C1", "1") != "0"
# lookups from which the once-per-flow build pays: build time / saving per lookup, rounded up -- 132.8 us / (69.4 - 30.6 us) = 3.4
# -> 4 at 1080p (profiles/lookup_band_ab.txt) -- and never below 6: below that the gain is inside the run-to-run spread, and
# short flows keep their launch programs
BAND_MIN_LOOKUPS = 6


def _ru(x, m):
    return (x + m - 1) // m * m


class Step(NamedTuple):
    """One entry of a launch program: what _Plan.run() dispatches on, its argument(s), the layer's name where it has one."""
    kind: str
    arg: object
    tag: str = None


class _Folded(NamedTuple):
    """The iteration programs with the flow-head gather that ends iteration k done by the lookup launch that starts iteration
    k + 1 (woft_lookup_otf_params.fh_*), the launch that closes the last iteration, and that lookup's parameter struct."""
    prog_iter_first: list
    prog_iter: list
    prog_iter_last: list       # None where the plan has no merged last iteration
    gather: list
    lookup: object


class FlowKey(NamedTuple):
    """What makes two _Plan.flow() calls the same launches on the same addresses: the key of a plan's captured graphs."""
    iters: int
    crop: tuple
    h: int
    w: int
    flow_up: int               # the outputs by address (None: not written)
    dst: int
    wout: int
    mout: int
    do_sigmoid: bool
    mask_sigmoid: bool
    defer_wh: bool
    skip_wh: bool
    has_init: bool             # a flow_init was given (its values are not part of the key: the graph reads the plan's buffer)
    target_restored: bool
    wh_region: int             # address of the weight region's window list (None: every source pixel)
    flow_region: tuple         # (rectangle, iterations) of the restricted iterations that run (None: none)


class _FlowGraph(torch.cuda.CUDAGraph):
    """A captured _Plan.flow() + post: the (band_valid, target_valid) that flow leaves in the plan, which a replay must set."""
    post = None


def _timed(sink, launch, *args, extra=None):
    """launch(*args); with a sink (a bench hook's list) between two HIP events, appended as (start, end[, extra()])."""
    if sink is None:
        return launch(*args)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    launch(*args)
    e.record()
    sink.append((s, e) if extra is None else (s, e, extra()))


def _head_layers(sd, prefix, cin):
    """Layers `prefix`0, `prefix`2, ... of a WeightHead / MaskHead in a state dict -> (their indices, their weight shapes, whether
    they form such a head on cin input channels: odd square kernels, matching channels, a closing 1x1 conv to one channel)."""
    idx = sorted(int(k.split(".")[2]) for k in sd if k.startswith(prefix) and k.endswith(".weight"))
    shapes = [tuple(sd[f"{prefix}{i}.weight"].shape) for i in idx]
    ok = not (len(idx) < 2 or shapes[-1][0] != 1 or shapes[-1][2:] != (1, 1) or shapes[0][1] != cin
              or any(a[0] != b[1] for a, b in zip(shapes, shapes[1:])) or any(sh[2] != sh[3] or sh[2] % 2 == 0 for sh in shapes))
    return idx, shapes, ok


class _Spec:
    """Architecture constants of the two model sizes (weighted_raft.py:34-72, raft.py:33-65)."""

    def __init__(self, small):
        self.small = small
        if small:
            self.fdim, self.hdim, self.cdim, self.radius = 128, 96, 64, 3
            self.fnorm, self.cnorm = "instance", "none"
        else:
            self.fdim, self.hdim, self.cdim, self.radius = 256, 128, 128, 4
            self.fnorm, self.cnorm = "instance", "batch"
        self.levels = 4
        self.nwin = 2 * self.radius + 1
        self.corr_c = self.levels * self.nwin ** 2            # 324 / 196
        self.corr_cs = _ru(self.corr_c, 32)                   # 352 / 224
        self.xdim = _ru(self.cdim + (82 if small else 128), 32)   # GRU input buffer [inp | motion | flow]
        self.flow_off = self.cdim + (80 if small else 126)    # channel of the flow inside that buffer


class _Enc:
    """Packed weights of one BasicEncoder / SmallEncoder (extractor.py:118-267)."""

    def __init__(self, sd, p, norm, spec, out_split=None):
        self.norm = norm

        def get(name, stride=1, flat_cs=0, bn=None):
            w, b = sd[name + ".weight"], sd[name + ".bias"]
            if norm == "batch" and bn is not None:
                w, b = ops.fold_bn(w, b, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"],
                                   sd[bn + ".running_var"])
            return ops.pack_conv(w, b, stride=stride, flat_cs=flat_cs)

        self.conv1 = get(p + ".conv1", 2, 4, p + ".norm1")
        self.blocks = []
        for li, stride in ((1, 1), (2, 2), (3, 2)):
            for bi in range(2):
                q = f"{p}.layer{li}.{bi}"
                s = stride if bi == 0 else 1
                if spec.small:      # BottleneckBlock, extractor.py:60-116: 1x1 -> 3x3(stride) -> 1x1
                    convs = [get(q + ".conv1", 1, bn=q + ".norm1"), get(q + ".conv2", s, bn=q + ".norm2"),
                             get(q + ".conv3", 1, bn=q + ".norm3")]
                else:               # ResidualBlock, extractor.py:6-56: 3x3(stride) -> 3x3
                    convs = [get(q + ".conv1", s, bn=q + ".norm1"), get(q + ".conv2", 1, bn=q + ".norm2")]
                blk = dict(stride=s, convs=convs)
                if s != 1:
                    blk["down"] = get(q + ".downsample.0", s, bn=q + ".downsample.1")
                self.blocks.append(blk)
        w2, b2 = sd[p + ".conv2.weight"], sd[p + ".conv2.bias"]
        if out_split:               # cnet: GRU state (tanh) and context (relu), weighted_raft.py:217-219
            self.conv2_net = ops.pack_conv(w2[:out_split], b2[:out_split])
            self.conv2_inp = ops.pack_conv(w2[out_split:], b2[out_split:])
        else:
            self.conv2 = ops.pack_conv(w2, b2)


class RaftEngine:
    def __init__(self, state_dict, small=False, weighted=True, precision="fp32", corr="volume", volume_storage=None,
                 mask_head=False, corr_band="auto", fuse_c1=True):
        """precision: "fp32" (exact fp32 MFMA), "bf16x3" (split-bf16, fp32-emulating), "bf16", or "fp16" = the reference's
        `mixed_precision` scoping (weighted_raft.py:204-219,233-234,258-290: autocast around fnet, cnet and the update block
        only): those convolutions on fp16 operands with fp32 accumulation, the correlation, the weight head and both
        upsamplings in fp32-class arithmetic (bf16x3 here).
        corr: "volume" (all-pairs volume + pyramid in HBM, corr.py:13-69) or "otf" (volume-free lookup from the
        feature maps, the reference's alternate_corr idea, corr.py:72-100; every precision, exact fp32 included: bit-identical
        to the volume path of the same precision).
        volume_storage: element type of the volume in HBM, "fp32" or "bf16" (fp32 accumulators rounded once at the GEMM's
        store; lookup interpolation and output stay fp32).  Default: "bf16" in the plain-bf16 precision -- its operating
        point, half the store stream and the lookup's reads, SURVEY 8d -- else "fp32".
        mask_head: also evaluate the MaskHead of a 'weighted_masked' checkpoint (mask_head.net.*, weighted_raft.py:295-309,387-422)
        after the last iteration -> flow(mout=...) receives the upsampled visibility logits."""
        if precision not in ops.PRECISION:
            raise ValueError(f"precision must be one of {sorted(ops.PRECISION)}")
        if corr not in ("volume", "otf"):
            raise ValueError("corr must be 'volume' or 'otf'")
        self.precision = precision
        # arithmetic of the correlation (volume GEMM / volume-free lookup) and of the weight head's convolutions
        # ("f16mx8": two matrix-pipe passes per product on the register-streamed conv kernel -- the update block; every other
        #  kernel, the correlation and the weight head run in bf16x3)
        self.prec_corr = self.prec_wh = "bf16x3" if precision in ("fp16", "f16mx8") else precision
        self.corr = corr
        if corr_band not in ("auto", True, False):
            raise ValueError("corr_band must be 'auto', True or False")
        self.corr_band = corr_band
        self.fuse_c1 = bool(fuse_c1)
        self.volume_storage = volume_storage or ("bf16" if precision == "bf16" else "fp32")
        if self.volume_storage not in ("fp32", "bf16") or (self.volume_storage == "bf16" and precision == "fp32"):
            raise ValueError("volume_storage: 'fp32', or 'bf16' with the split-bf16 precisions (their GEMM packs it)")
        _lib.load()
        if not torch.cuda.is_available():
            raise _lib.WoftHipError("woft_amd needs a HIP device: there is no CPU fallback")
        sd = {k: v.detach().float().cpu() for k, v in state_dict.items()}
        self.weighted, self.small, self.mask_head = weighted, small, bool(mask_head)
        self.spec = sp = _Spec(small)
        self.radius, self.levels = sp.radius, sp.levels
        if self.mask_head and not weighted:
            raise ValueError("mask_head: the MaskHead belongs to WeightedRAFT (weighted_raft.py:75-76), not to plain RAFT")
        # (what only some models have: the full model's second correlation conv and upsampling-mask head, the two heads)
        self.convc2 = self.mk1 = self.mk2 = None
        self.wh_std = self.wh_flat0 = False
        self.wh0 = self.wh2 = self.wh4 = self.wh0_frag = self.wh_layers = self.wh6_c = self.wh6_w = self.wh6_b = None
        self.mh_shapes = self.mh_layers = self.mh_c = self.mh_wlast = self.mh_b = None
        self._pack_encoders(sd)
        self._pack_update_block(sd)
        if weighted:
            self._pack_weight_head(sd)
        if self.mask_head:
            self._pack_mask_head(sd)
        self._plans = {}

    def _pack_encoders(self, sd):
        self.fnet = _Enc(sd, "fnet", self.spec.fnorm, self.spec)
        self.cnet = _Enc(sd, "cnet", self.spec.cnorm, self.spec, out_split=self.spec.hdim)

    def _pack_update_block(self, sd):
        sp, small, precision = self.spec, self.small, self.precision
        u = "update_block."
        g = lambda n, **kw: ops.pack_conv(sd[u + n + ".weight"], sd[u + n + ".bias"], **kw)
        self.convc1 = g("encoder.convc1")
        self.convf1 = g("encoder.convf1", flat_cs=4)
        self.convf2 = g("encoder.convf2")
        self.convm = g("encoder.conv")
        self.fh1 = g("flow_head.conv1")
        self.fh2 = g("flow_head.conv2")
        # second conv of the flow head as MFMA fragments: folded into the first conv's epilogue (WOFT_EPI_FLOWHEAD)
        self.fh2_frag = (ops.pack_flowhead_frags(sd[u + "flow_head.conv2.weight"], 2 if precision in ("bf16x3", "f16mx8") else 1,
                                                 f16=precision == "fp16")
                         if precision != "fp32" and FUSE_FLOWHEAD else None)
        if not small:
            self.convc2 = g("encoder.convc2")
            self.mk1 = g("mask.0")
            self.mk2 = g("mask.2", scale=0.25)         # ".25 * self.mask(net)"  update.py:135
        # The GRU convs see [h | inp | motion] (update.py:22-31, 45-60, 127-131) and `inp` (the context features) is the
        # same in every iteration: conv(W, [h, inp, motion]) = conv(W_[h,motion], [h, motion]) + conv(W_inp, inp).
        # The second term (+ bias) is computed once per source image (zr_inp / q_inp -> the plan's gate_bias) and enters the
        # iterations as a per-pixel bias; the per-iteration convs (zr_dyn / q_dyn) run without the context channels.
        # One entry per GRU (half) step: the small model's single 3x3 step, the full model's 1x5 and 5x1 steps.
        hd_, cd_, mot = sp.hdim, sp.cdim, (82 if small else 128)
        dyn = [(0, hd_, 0), (hd_ + cd_, hd_ + cd_ + mot, hd_)]              # h -> 0.., motion(+flow) -> hd..
        ctx = [(hd_, hd_ + cd_, 0)]
        self.zr_dyn, self.zr_inp, self.q_dyn, self.q_inp = [], [], [], []
        for sfx, pd in (("", None),) if small else (("1", (0, 2)), ("2", (2, 0))):
            zr_w, zr_b = (torch.cat([sd[f"{u}gru.convz{sfx}{s}"], sd[f"{u}gru.convr{sfx}{s}"]], 0) for s in (".weight", ".bias"))
            q_w, q_b = sd[f"{u}gru.convq{sfx}.weight"], sd[f"{u}gru.convq{sfx}.bias"]
            self.zr_dyn.append(ops.pack_conv(zr_w, None, padding=pd, cin_layout=dyn))
            self.zr_inp.append(ops.pack_conv(zr_w, zr_b, padding=pd, cin_layout=ctx))
            self.q_dyn.append(ops.pack_conv(q_w, None, padding=pd, cin_layout=dyn))
            self.q_inp.append(ops.pack_conv(q_w, q_b, padding=pd, cin_layout=ctx))

    def _pack_weight_head(self, sd):
        sp, precision = self.spec, self.precision
        w = "weight_head.net."
        # class_params.weight_head_structure (weighted_raft.py:318-345) = the state-dict's layers net.0, net.2, ..., a ReLU after
        # each, then the closing 1x1 conv.  The shipped configs' [(128, 3)] * 3 (optical_flow/configs/v2_SNOB_large_g05_RAFT.py:16)
        # has its own kernels (first layer fused into the second's launch, mean fused into the third's epilogue, evaluated on
        # a subset of the windows); any other structure runs layer by layer on every window (wh_std = False).
        idx, shapes, ok = _head_layers(sd, w, sp.levels + 1)
        if not ok:
            raise ValueError(f"weight head layers {shapes}: not a WeightHead (weighted_raft.py:318-345)")
        self.wh_std = shapes == [(128, 5, 3, 3), (128, 128, 3, 3), (128, 128, 3, 3), (1, 128, 1, 1)]
        last = idx[-1]
        if self.wh_std:
            self.wh0, self.wh2, self.wh4, self.wh0_frag = self._wh_std_packed(sd)
        else:
            # generic head: the first layer reads the 5-channel patches -- "flat" packing (8 floats per window position)
            # while kernel * 8 <= 32, else 32-channel rows; the other layers are ordinary convs on (windows, n, n, C)
            k0 = shapes[0][2]
            self.wh_flat0 = k0 * 8 <= 32
            self.wh_layers = [ops.pack_conv(sd[f"{w}{idx[0]}.weight"], sd[f"{w}{idx[0]}.bias"], flat_cs=8 if self.wh_flat0 else 0)]
            self.wh_layers += [ops.pack_conv(sd[f"{w}{i}.weight"], sd[f"{w}{i}.bias"]) for i in idx[1:-1]]
        self.wh6_c = shapes[-1][1]
        self.wh6_w = torch.zeros(_ru(self.wh6_c, 4))
        self.wh6_w[:self.wh6_c] = sd[f"{w}{last}.weight"].reshape(-1)
        self.wh6_w = self.wh6_w.contiguous().cuda()
        self.wh6_b = float(sd[f"{w}{last}.bias"].item())

    def _wh_std_packed(self, sd):
        """The three 3x3 layers of the standard head packed for the conv kernels -> (wh0, wh2, wh4, wh0_frag)."""
        w = "weight_head.net."
        wh0 = ops.pack_conv(sd[w + "0.weight"], sd[w + "0.bias"], flat_cs=8)
        wh2 = ops.pack_conv(sd[w + "2.weight"], sd[w + "2.bias"])
        wh4 = ops.pack_conv(sd[w + "4.weight"], sd[w + "4.bias"])
        # first conv as MFMA fragments for the fused two-layer launch (split-bf16 precisions, 9x9 windows)
        wh0_frag = (ops.pack_wh0_frags(sd[w + "0.weight"], 2 if self.prec_wh == "bf16x3" else 1)
                    if self.precision != "fp32" and self.spec.nwin == 9 else None)
        return wh0, wh2, wh4, wh0_frag

    def repack_weight_head(self, sd):
        """Re-pack the standard head from `sd` (its eight weight_head.net.* tensors) IN PLACE into every device buffer the
        inference path reads head parameters from -- the engine's packed layers and fragments, the closing conv's weights and
        bias, and every plan's own copies (_Plan.refresh_weight_head, which also drops the plan's captured graphs).  The next flow
        then has the bits of an engine built from `sd`."""
        assert self.weighted and self.wh_std
        sd = {k: v.detach().float().cpu() for k, v in sd.items() if k.startswith("weight_head.net.")}
        wh0, wh2, wh4, frag = self._wh_std_packed(sd)
        for old, new in ((self.wh0, wh0), (self.wh2, wh2), (self.wh4, wh4)):
            ops.repack_conv_(old, new)
        if self.wh0_frag is not None:
            self.wh0_frag.copy_(frag)
        self.wh6_w[:self.wh6_c].copy_(sd["weight_head.net.6.weight"].reshape(-1))
        self.wh6_b = float(sd["weight_head.net.6.bias"].item())
        for plan in self._plans.values():
            plan.refresh_weight_head()

    def _pack_mask_head(self, sd):
        sp = self.spec
        m = "mask_head.net."
        # class_params.mask_head_structure (weighted_raft.py:387-409) = the layers net.0, net.2, ... on [fmap1 | warped fmap2]
        # (2 * fdim channels), a ReLU after each, then the closing 1x1 conv to one logit channel
        idx, shapes, ok = _head_layers(sd, m, 2 * sp.fdim)
        if not ok:
            raise ValueError(f"mask head layers {shapes}: not a MaskHead on {2 * sp.fdim} channels (weighted_raft.py:387-409)")
        self.mh_shapes = shapes
        self.mh_c = shapes[-1][1]
        self.mh_layers, self.mh_wlast, self.mh_b = self._mh_packed(sd, idx)

    @staticmethod
    def _mh_packed(sd, idx):
        """The MaskHead's layers net.{idx} of `sd` packed for the conv kernels -> (mh_layers, mh_wlast, mh_b)."""
        m = "mask_head.net."
        layers = [ops.pack_conv(sd[f"{m}{i}.weight"], sd[f"{m}{i}.bias"]) for i in idx[:-1]]
        return layers, sd[f"{m}{idx[-1]}.weight"].reshape(-1).clone(), float(sd[f"{m}{idx[-1]}.bias"].item())

    def repack_mask_head(self, sd):
        """Re-pack the MaskHead from `sd` (its mask_head.net.* tensors) IN PLACE into every device buffer the inference path reads
        head parameters from -- the engine's packed layers in every form they have, the closing conv's weights and bias, and every
        plan's own copy (_Plan.refresh_mask_head, which also drops the plan's captured graphs: a captured launch bakes the closing
        bias in as an argument).  The next flow then has the bits of an engine built from `sd`."""
        assert self.mask_head
        sd = {k: v.detach().float().cpu() for k, v in sd.items() if k.startswith("mask_head.net.")}
        layers, wlast, b = self._mh_packed(sd, list(range(0, 2 * len(self.mh_shapes), 2)))
        for old, new in zip(self.mh_layers, layers):
            ops.repack_conv_(old, new)
        self.mh_wlast.copy_(wlast)
        self.mh_b = b
        for plan in self._plans.values():
            plan.refresh_mask_head()

    def plan(self, hp, wp, slot=0):
        """Buffers + launch programs for one padded input size.  slot: an independent second set for the same size (the
        flow provider keeps a pinned source image -- the tracker's template -- resident in slot 0 and runs flows from other
        sources, the tracker's frame t-1 -> t flow of a lost frame, in slot 1: 5 GB more at 1080p, of 288)."""
        key = (hp, wp) if slot == 0 else (hp, wp, slot)
        if key not in self._plans:
            self._plans[key] = _Plan(self, hp, wp)
        return self._plans[key]

    def drop_plan(self, key):
        """Forget the plan stored under `key` (the key `plan()` files it under) and with it its buffers; -> the plan or None.
        Nobody calls this unless asked to bound the number of shapes (RAFTWrapper.bound_plans)."""
        return self._plans.pop(key, None)


class _Plan:
    """Buffers + launch programs for one padded input size (hp, wp), both multiples of 8."""

    def __init__(self, eng, hp, wp):
        assert hp % 8 == 0 and wp % 8 == 0
        self.eng, self.hp, self.wp = eng, hp, wp
        self.prec, self.prec_corr, self.prec_wh = eng.precision, eng.prec_corr, eng.prec_wh
        self.otf = eng.corr == "otf"
        self.hf, self.wf, self.P = hp // 8, wp // 8, (hp // 8) * (wp // 8)
        # what the operand buffers hold (_source_changed / _target_changed): source_owner = the (tag, key) that claimed the source
        # state at encode_source(); target_owner = the token the target image was loaded under; target_valid = the level-0 target
        # map + operand are that image's (flow() sets it); band_valid = the band holds the current operands' correlations
        self._source_changed()
        self._target_changed()
        self.lookup_events = None  # bench hook: list collecting (start, end) HIP events per lookup launch
        self.wh_events = None      # bench hook: (start, end, windows) around the weight head's first 128->128 layer
        self.conv_events = None    # bench hook: {tag: [(start, end)]} for the tagged conv launches of the iteration program
        self._graphs = {}          # flow(graph=True): {FlowKey: its _FlowGraph, or None after the first sighting}
        # correlation band: its buffers (first use) and the band variants of the lookup parameter structs (by the address of the
        # volume-free struct they mirror)
        self._band = None
        self._band_params = {}
        self._fuse_c1 = False      # this flow's iterations may run convc1 on the band (set by _flow: never under a trace)
        # what only some plans have: the full model's upsampling mask, a merged last iteration, the folded programs, fh_part (flow
        # head folded into one conv launch: per-pixel partial products of its second conv), the two heads
        self.mk = self.mask = self.prog_iter_last = self.folded = self.fh_part = None
        self.x8 = self.x32 = self.wmean = self.wlow = self.cs_ws = self.cs_tot = self.wh6_b = self._wh6_pad = None
        self.a1 = self.a2 = self.wh0_t = self.wh_last = None
        self.wh0_direct = self.wh0_fused = self.wh_fused = False
        self.prog_mask, self.prog_wh, self.prog_mh = [], [], []
        self.mh_warped = self.mh_last = self.mh_w = self.mh_low = None
        self.flow_region, self._flow_regions = None, {}        # None = every launch on the whole map (set_flow_region)
        self.wh_region, self._wh_regions = None, {}            # None = every source pixel (set_weight_region)
        self._wh_dyn = {}                                      # per region: (dynamic window list, its programs, scratch)
        self._wh_train = None                                  # buffers of wh_train_forward / wh_train_backward (first use)
        self._mh_train = None                                  # buffers of mh_train_forward / mh_train_backward (first use)
        self._plan_features()
        self._plan_update_block()
        if eng.weighted:
            self._plan_weight_head()
        if eng.mask_head:
            self._plan_mask_head()

    @staticmethod
    def _z(*s, dtype=torch.float32):
        return torch.zeros(*s, dtype=dtype, device="cuda")

    def _plan_features(self):
        """Images, feature maps, the target pyramid / volumes, the context buffers; the encoder and volume programs."""
        eng, sp, hp, wp, hf, wf, P, z = self.eng, self.eng.spec, self.hp, self.wp, self.hf, self.wf, self.P, self._z
        self.img = [new_act(1, hp, wp, 3, cs=4), new_act(1, hp, wp, 3, cs=4)]
        # source features: rows padded to the 128-row GEMM tile (pad rows stay zero), + their bf16 hi/lo planes
        self.f1rows = z(_ru(P, 128), sp.fdim)
        self.f1 = Act(self.f1rows[:P], 1, hf, wf, sp.fdim)
        x3 = self.prec_corr == "bf16x3"
        bf = lambda rows: (z(rows.shape[0], rows.shape[1] * (2 if x3 else 1), dtype=torch.bfloat16)
                           if self.prec != "fp32" else None)       # GEMM operand: [hi|lo] lines / bf16 plane
        self.f1s = bf(self.f1rows)
        if self.otf and self.prec == "fp32":
            self.f1s = self.f1rows      # exact fp32 (terms = 0): the volume-free lookup reads the fp32 feature rows themselves
        # target feature pyramid: linear NHWC maps (f2act) and their rows in 4x4-tile order (f2rows, the B
        # operand of the correlation GEMM, zero padded to the N tile) -> volumes in the tiled layout
        # (corr = "otf": no volume; the lookup reads the row-major split maps f2s directly)
        self.dims, self.f2rows, self.f2act, self.vol, self.f2s = [], [], [], [], []
        h, w = hf, wf
        for _ in range(sp.levels):
            self.dims.append((h, w))
            self.f2act.append(new_act(1, h, w, sp.fdim, zero=True))
            if self.otf:
                self.f2s.append(bf(self.f2act[-1].t) if self.prec != "fp32" else self.f2act[-1].t)
            else:
                n = ops.tiled_dims(h, w)[2]
                rows = z(_ru(n, 128), sp.fdim)
                self.f2rows.append(rows)
                self.f2s.append(bf(rows))
                self.vol.append(z(P, n, dtype=torch.bfloat16 if eng.volume_storage == "bf16" else torch.float32))
            h, w = h // 2, w // 2
        # context: GRU state and the GRU input buffer [inp | motion | flow | pad]; flow_cat = its flow channels onwards
        self.net0 = new_act(1, hf, wf, sp.hdim, zero=True)
        self.xbuf = new_act(1, hf, wf, sp.xdim, zero=True)
        self.flow_cat = self.xbuf.t[:, sp.flow_off:]
        self._enc_scratch = {}
        n_stat = 2 * math.ceil((hp // 2) * (wp // 2) / 64) * 128
        self.stats = (z(n_stat), z(n_stat))
        self.fin_ws = ops.inorm_ws("cuda")
        self._norm_slots = {}
        self.prog_f_src = self._encoder_program(eng.fnet, self.img[0], [(eng.fnet.conv2, self.f1, 0, EPI.EPI_LINEAR)])
        self.prog_f_dst = self._encoder_program(eng.fnet, self.img[1],
                                                [(eng.fnet.conv2, self.f2act[0], 0, EPI.EPI_LINEAR)])
        self.prog_c_src = self._encoder_program(eng.cnet, self.img[0],
                                                [(eng.cnet.conv2_net, self.net0, 0, EPI.EPI_TANH),
                                                 (eng.cnet.conv2_inp, self.xbuf, 0, EPI.EPI_RELU)])
        self.prog_volume = self._volume_program()

    def _plan_update_block(self):
        """Buffers of the refinement loop, the lookup's parameters, the iteration programs and the upsampling-mask convs."""
        eng, sp, hf, wf, P, z, cp = self.eng, self.eng.spec, self.hf, self.wf, self.P, self._z, self._cp
        self.coords = z(P, 2)
        self.corr = new_act(1, hf, wf, sp.corr_c, cs=sp.corr_cs, zero=True)
        self.c1 = new_act(1, hf, wf, 96 if sp.small else 256, zero=True)
        self.cf = new_act(1, hf, wf, 128 if sp.small else 256, zero=True)     # [cor | flo]
        self.fl1 = new_act(1, hf, wf, 64 if sp.small else 128, zero=True)
        self.flow4 = new_act(1, hf, wf, 2, cs=4, zero=True)
        # per-pixel gate biases conv(W_inp, inp) + b: z|r and q of every GRU (half) step ([h | motion] convs: see RaftEngine)
        self.inp_c = new_act(1, hf, wf, sp.cdim, zero=True)
        self.gate_bias = [(new_act(1, hf, wf, 2 * sp.hdim, zero=True), new_act(1, hf, wf, sp.hdim, zero=True))
                          for _ in eng.zr_inp]
        self.prog_gate_bias = []
        for k in range(len(eng.zr_inp)):
            self.prog_gate_bias += [Step("conv", cp(self.inp_c, eng.zr_inp[k], self.gate_bias[k][0])),
                                    Step("conv", cp(self.inp_c, eng.q_inp[k], self.gate_bias[k][1]))]
        self.zbuf = new_act(1, hf, wf, sp.hdim, zero=True)
        self.rh = new_act(1, hf, wf, sp.hdim, zero=True)
        self.hA = new_act(1, hf, wf, sp.hdim, zero=True)
        self.hB = new_act(1, hf, wf, sp.hdim, zero=True)
        self.fh = new_act(1, hf, wf, 128 if sp.small else 256, zero=True)
        self.delta = new_act(1, hf, wf, 2, cs=4, zero=True)
        # warm start: the caller's flow_init is copied here, so that a captured graph reads it from a fixed address
        self.flow_init = z(2, hf, wf)
        if self.otf:
            terms = 3 if self.prec_corr == "bf16x3" else (0 if self.prec == "fp32" else 1)
            self.lookup = ops.make_lookup_otf_params(self.f1s, self.f2s, self.dims, hf, wf, sp.fdim, self.coords,
                                                     self.corr.t, sp.radius, terms)
        else:
            self.lookup = ops.make_lookup_params(self.vol, self.dims, self.coords, self.corr.t, sp.radius)
        self.prog_iter_first = self._iter_program(first=True)
        self.prog_iter = self._iter_program(first=False)
        if not sp.small:
            self.mk = new_act(1, hf, wf, 256, zero=True)
            self.mask = new_act(1, hf, wf, 576, zero=True)
            # (prog_mask, prog_wh and prog_mh are lists of conv parameter structs, not of Steps: flow() and the heads launch
            #  them one by one, and the benchmark's roofline and the tests read the structs' fields)
            self.prog_mask = [cp(self.hB, eng.mk1, self.mk, epi=EPI.EPI_RELU),
                              cp(self.mk, eng.mk2, self.mask)]
            # last iteration: the flow head's conv and the mask head's first conv both read the final GRU state and are
            # independent (update.py:132-135) -> one launch when they select the same kernel instance (woft_conv2d_pair)
            k = next((i for i, st in enumerate(self.prog_iter) if st.tag == "fh1"), None)
            if PAIR_BRANCHES and k is not None and ops.pair_ok(self.prog_iter[k].arg, self.prog_mask[0]):
                self.prog_iter_last = (self.prog_iter[:k] + [Step("conv2", (self.prog_iter[k].arg, self.prog_mask[0]), "fh1+mk1")]
                                       + self.prog_iter[k + 1:])
        self.folded = self._fold_gather_programs()

    def _plan_weight_head(self):
        eng, sp, P, z, n = self.eng, self.eng.spec, self.P, self._z, self.eng.spec.nwin
        self.x8 = new_act(P, n, n, 5, cs=8, zero=True)
        self.wmean = z(P)
        self.wlow = z(P)
        self.cs_ws = z(256, sp.fdim, dtype=torch.float64)
        self.cs_tot = z(sp.fdim, dtype=torch.float64)
        self.wh6_b = torch.tensor([eng.wh6_b], dtype=torch.float32, device="cuda")
        cpw = lambda *a, **kw: self._cp(*a, precision=self.prec_wh, **kw)
        if eng.wh_std:
            self.a2 = new_act(P, n, n, 128)
            # first conv (5 -> 128): scalar-operand VALU kernel straight from the lookup buffer for the 7x7 / 9x9
            # windows (woft_wh_conv0), the generic conv on the packed x8 patches otherwise
            self.wh0_direct = n in (7, 9)
            self.wh0_fused = (eng.wh0_frag is not None and os.environ.get("WOFT_WH0_FUSED", "1") != "0"
                              and ops.select_conv(self.a2, eng.wh2, precision=self.prec_wh).kernel is Kernel.WINDOW_9X9)
            # (with the first layer AND the tail fused into the two 128->128 launches only ONE activation exists)
            self.a1 = self.a2 if self.wh0_fused else new_act(P, n, n, 128)
            self.wh0_t = eng.wh0.wgt[:128].t().contiguous()          # [ky*32 + kx*8 + ci][co]
            # (the head restricted to a subset of the source pixels -- set_weight_region -- has its own programs per region)
            self.prog_wh, self.wh_fused = self._wh_program(P, None)
            return
        # any other weight_head_structure: layer by layer on every window, the closing 1x1 conv + window mean by
        # woft_wh_reduce (no window subsets, no fused layers: a correct path, not a tuned one)
        x = self.x8
        if not eng.wh_flat0:                     # first kernel wider than 3: 32-channel rows instead of the flat 8
            self.x32 = x = new_act(P, n, n, 5, cs=32, zero=True)
        # one activation per layer, zeroed once: a layer writes its cout channels only, so the pad channels that the next
        # layer's 32-channel K chunks (and woft_wh_reduce) read against zero weights stay exact zeros for ever -- a buffer
        # shared between layers of different widths would show a narrower layer what a wider one left behind (0 * inf = NaN)
        for pc in eng.wh_layers:
            out = new_act(P, n, n, pc.cout, cs=_ru(_ru(pc.cout, 4), 32), zero=True)
            self.prog_wh.append(cpw(x, pc, out, epi=EPI.EPI_RELU))
            x = out
        self.wh_last = x

    def _plan_mask_head(self):
        # MaskHead (weighted_raft.py:295-309,387-422), after the last iteration on every source pixel (3x3 cross-pixel terms):
        # woft_warp_features -> layers on the conv kernels (the first reads [f1 | warped] as two sources, no concatenated copy)
        # -> closing 1x1 conv by woft_wh_reduce (nwin2 = 1) -> 1/8-resolution logits mh_low.  Arithmetic: the weight head's
        # rule (prec_wh; the reference runs the head outside autocast).  One activation per layer, zeroed once (_plan_weight_head).
        eng, sp, hf, wf = self.eng, self.eng.spec, self.hf, self.wf
        self.mh_warped = new_act(1, hf, wf, sp.fdim, zero=True)
        x = None
        for k, pc in enumerate(eng.mh_layers):
            out = new_act(1, hf, wf, pc.cout, cs=_ru(_ru(pc.cout, 4), 32), zero=True)
            src = dict(x2=self.mh_warped, c_split=sp.fdim) if k == 0 else {}
            self.prog_mh.append(self._cp(self.f1 if k == 0 else x, pc, out, epi=EPI.EPI_RELU, precision=self.prec_wh, **src))
            x = out
        self.mh_last = x
        self.mh_w = torch.zeros(x.cs, dtype=torch.float32)
        self.mh_w[:eng.mh_c] = eng.mh_wlast
        self.mh_w = self.mh_w.to("cuda")
        self.mh_low = self._z(self.P)

    def _fold_gather_programs(self):
        """-> the _Folded variants of the iteration programs, or None (switched off, the volume lookup, an unfused flow head)."""
        progs = [p for p in (self.prog_iter_first, self.prog_iter, self.prog_iter_last) if p is not None]
        if not (FOLD_GATHER and self.otf and all(p and p[-1].kind == "fh_gather" and p[0].kind == "lookup" for p in progs)):
            return None
        n_planes, bias2 = self.prog_iter[-1].arg
        lk = ops.copy_params(self.lookup)
        lk.fh_part, lk.fh_bias, lk.fh_delta = _lib.ptr(self.fh_part), _lib.ptr(bias2), _lib.ptr(self.delta.t)
        lk.fh_flow4, lk.fh_flow_cat = _lib.ptr(self.flow4.t), self.flow_cat.data_ptr()
        lk.fh_planes, lk.fh_ld, lk.fh_ld_delta, lk.fh_ld_cat = n_planes, self.fh_part.shape[1], self.delta.cs, self.xbuf.cs
        lk._keep = (self.lookup._keep, bias2, self.fh_part)
        # (the first iteration's lookup has no gather before it)
        first, mid, last = ([head] + p[1:-1] if p is not None else None
                            for p, head in ((self.prog_iter_first, self.prog_iter_first[0]), (self.prog_iter, Step("lookup", lk)),
                                            (self.prog_iter_last, Step("lookup", lk))))
        return _Folded(first, mid, last, [self.prog_iter[-1]], lk)

    def _wh_program(self, n_win, index):
        """Launch list of the head's 128->128 layers on n_win windows (all source pixels, or those listed in the
        int32 tensor `index`) -> (program, fused): fused = the last layer runs on the whole-window kernel with
        ReLU + 1x1 conv + window mean in its epilogue."""
        eng, n = self.eng, self.eng.spec.nwin
        cp = lambda *a, **kw: self._cp(*a, precision=self.prec_wh, **kw)          # (fp32-class also in the fp16 mode)
        a1 = Act(self.a1.t[:n_win * n * n], n_win, n, n, 128)
        a2 = Act(self.a2.t[:n_win * n * n], n_win, n, n, 128)
        prog = ([] if self.wh0_direct else [cp(self.x8, eng.wh0, a1, epi=EPI.EPI_RELU)]) + [
            cp(a1, eng.wh2, a2, epi=EPI.EPI_RELU), cp(a2, eng.wh4, a1, epi=EPI.EPI_RELU)]
        if self.wh0_fused:          # layers 1 + 2 in one launch: the first activation (1.3 GB at 1080p) never exists
            assert Kernel(prog[0].halo) is Kernel.WINDOW_9X9
            prog[0] = cp(a1, eng.wh2, a2, epi=EPI.EPI_RELU,
                         wh0=(self.corr, self.wmean, eng.wh0_frag, eng.wh0.bias, index))
        last = prog[-1]
        fused = Kernel(last.halo) is Kernel.WINDOW_9X9
        if fused:
            last.epi = EPI.EPI_WH_MEAN
            last.e0, last.e1 = _lib.ptr(eng.wh6_w), _lib.ptr(self.wh6_b)
            last.out, last.ldo, last.co_off = _lib.ptr(self.wlow), 1, 0
            last.out_index = _lib.ptr(index) if index is not None else None
        return prog, fused

    def set_weight_region(self, index):
        """Evaluate the weight head only on the source pixels listed in `index` (int32 device tensor of 1/8-res
        pixel ids, or None for all): the other entries of the low-res weight map are zero.  Per-pixel results
        are unchanged (the head has no cross-pixel terms, weighted_raft.py:363-383); callers pass the pixels whose
        weights they consume (the tracker: its template mask, TRK:287-312, dilated by the upsampling support)."""
        if index is None or not (self.eng.weighted and self.wh0_direct and self.wh_fused):
            self.wh_region = None
            return
        key = index.data_ptr()
        if key not in self._wh_regions:
            prog, fused = self._wh_program(int(index.numel()), index)
            assert fused
            self._wh_regions[key] = (index, prog)
        self.wh_region = self._wh_regions[key]

    # ---- the refinement loop restricted to what a rectangle of the flow depends on -----------------
    def _layer_taps(self):
        """{layer: (reach along y, along x)} of the update block's convs, from the packed layers themselves."""
        e = self.eng
        r = lambda pc: (flow_region.reach(pc.kh or pc.taps_y, pc.pad_y), flow_region.reach(pc.kw or pc.taps_x, pc.pad_x))
        return {"convc1": r(e.convc1), "convc2": r(e.convc2), "convf1": r(e.convf1), "convf2": r(e.convf2), "convm": r(e.convm),
                "gru0": r(e.zr_dyn[0]), "gru1": r(e.zr_dyn[1]), "fh1": r(e.fh1), "fh2": r(e.fh2), "mk1": r(e.mk1), "mk2": r(e.mk2)}

    def set_flow_region(self, rect, iters=None):
        """The caller reads the full-resolution flow (flow_up / dst, and the weights) of the next flow() of `iters` iterations only
        inside the 1/8-resolution cells rect = (y0, x0, h, w) (None: everywhere).  The launches of the last iterations are then
        restricted to the rectangles those cells depend on (woft_amd/flow_region.py: derived backwards from the convex
        upsampling's 3x3 support, layer by layer, from the layers' own taps); an iteration whose every rectangle is the whole map
        runs today's program objects.  Inside the rectangle's pixels the results are bit-identical to the unrestricted flow;
        outside they are unspecified but finite (as the weights outside finish_weights()' pixels).  Programs are built once per
        (rectangle, iteration count).  Full model on the volume-free correlation with the folded flow head only -- anything else
        (and a trace, or a warm start, in flow()) runs every launch on the whole map; -> whether anything is restricted."""
        self.flow_region = None
        sp = self.eng.spec
        if rect is None or iters is None or iters < 2 or sp.small or not self.otf or self.folded is None \
                or self.prog_iter_last is None or len(self.eng.zr_dyn) != 2:
            return False
        key = (tuple(int(v) for v in rect), int(iters))
        if key not in self._flow_regions:
            self._flow_regions[key] = self._flow_region_programs(*key, [self._iteration(it, key[1], True) for it in range(key[1])])
        self.flow_region = self._flow_regions[key]
        return self.flow_region is not None

    def _iteration(self, it, iters, folded):
        """The launch program of refinement iteration `it` of `iters` (folded: from the set whose gathers run inside the next
        iteration's lookup).  The merged last program is an iteration of its own kind: a single iteration is a first one."""
        progs = self.folded if folded else self
        if it == 0:
            return progs.prog_iter_first
        if it == iters - 1 and progs.prog_iter_last is not None:
            return progs.prog_iter_last
        return progs.prog_iter

    def _flow_region_programs(self, rect, iters, base):
        """base: the unrestricted (folded) program of every iteration -> {"key", "iters": {iteration: restricted program},
        "rects": [(iteration, tag, [rect per part])]} or None when no launch is smaller than the whole map."""
        hf, wf = self.hf, self.wf
        taps = self._layer_taps()
        parts = {}
        for first in (True, False):
            for _, pp in flow_region.iteration_launches(taps, first=first, last=True, folded=True):
                for part in pp:
                    parts[(first, part[0])] = part
        launches, where = [], []
        for it in range(iters):
            for k, st in enumerate(base[it]):
                if st.kind == "lookup":
                    names = (["gather"] if st.arg.fh_part else []) + ["lookup"]
                elif st.kind in ("conv", "conv2") and st.tag is not None:
                    names = st.tag.split("+")
                else:
                    return None                              # (a launch this derivation does not know: nothing is restricted)
                if any((it == 0, n) not in parts for n in names):
                    return None
                launches.append((it, st.tag or "lookup", [parts[(it == 0, n)] for n in names]))
                where.append((it, k))
        launches += [(-1, tag, pp) for tag, pp in flow_region.closing_launches(taps)]
        rects, _ = flow_region.schedule(launches, flow_region.final_need(rect, hf, wf), hf, wf)

        def tiles(kernel, r):
            """Workgroups per column tile of a launch on rectangle r (None: the whole map): a conv kernel's, or the lookup's 8x8 blocks."""
            if kernel is not None:
                return conv_select.roi_tiles(kernel, r, hf, wf)
            y0, x0, h, w = r or (0, 0, hf, wf)
            return (-(-(y0 + h) // 8) - y0 // 8) * (-(-(x0 + w) // 8) - x0 // 8)

        # a rectangle is handed to a kernel only where it saves a tenth of the launch's workgroups: a launch may always compute more
        # than it must, and e.g. 64-pixel runs along the rows of a rectangle a little narrower than the map are MORE workgroups
        # than the map's linear tiling (measured slower: profiles/flow_region_ab.txt)
        small = lambda r, kernel=None: (r is not None and not flow_region.is_full(r, hf, wf)
                                        and 10 * tiles(kernel, r) <= 9 * tiles(kernel, None))
        roi = lambda p: KERNELS[Kernel(p.halo)].roi              # (the kernel takes an output rectangle: woft_conv_params.roi_*)

        def restricted(p, r):
            q = ops.copy_params(p)
            q.roi_y0, q.roi_x0, q.roi_h, q.roi_w = r
            return q

        progs = {}
        for (it, k), (_, tag, _), rr in zip(where, launches, rects):
            st = base[it][k]
            new = None
            if st.kind == "lookup" and small(rr[-1]):
                lk = restricted(st.arg, rr[0])               # launched blocks: the gather's pixels (or, without one, the samples')
                lk.smp_y0, lk.smp_x0, lk.smp_h, lk.smp_w = rr[-1]
                new = Step("lookup", lk)
            elif st.kind == "conv" and roi(st.arg) and small(rr[0], Kernel(st.arg.halo)):
                new = Step("conv", restricted(st.arg, rr[0]), tag + "@roi")
            elif st.kind == "conv2" and roi(st.arg[0]) and any(small(r, Kernel(st.arg[0].halo)) for r in rr):
                new = Step("conv2", tuple(restricted(p, r) if small(r, Kernel(p.halo)) else p for p, r in zip(st.arg, rr)), tag + "@roi")
            if new is not None:
                progs.setdefault(it, list(base[it]))[k] = new
        if not progs:
            return None
        return {"key": (rect, iters), "iters": progs,
                "rects": [(it, tag, rr) for (it, tag, _), rr in zip(launches, rects)]}

    def _cp(self, *a, **kw):
        kw.setdefault("precision", self.prec)
        return ops.conv_params(*a, **kw)

    # ---- encoders ------------------------------------------------------------------------
    def _scratch(self, name, n, h, w, c):
        cs = _ru(c, 32)                       # every encoder activation is a conv input: whole K chunks
        key = (name, h, w, cs)
        if key not in self._enc_scratch:
            self._enc_scratch[key] = new_act(n, h, w, c, cs=cs, zero=True)
        return self._enc_scratch[key]

    def _encoder_program(self, e, img, outputs):
        """extractor.py:168-192 / 244-267.  InstanceNorm: conv (+ partial statistics) -> finalize ->
        normalise/relu(/residual) kernels.  BatchNorm(eval, folded) / no norm: everything in conv epilogues."""
        prog = []
        inorm = e.norm == "instance"
        tag = "i" if inorm else "c"

        def slot(name):
            """(mean, rstd) buffers of one normalised layer: a deferred normalisation may be consumed several launches later."""
            key = f"{tag}_{name}"
            if key not in self._norm_slots:
                self._norm_slots[key] = (torch.zeros(256, device="cuda"), torch.zeros(256, device="cuda"))
            return self._norm_slots[key]

        def materialise(x):
            """A pending activation ("raw", act, mode, stats[, cache]) -> its normalised tensor (apply kernel; once)."""
            if not isinstance(x, list):
                return x
            if x[4] is None:
                _, raw_x, mode, ms, _ = x
                x[4] = self._scratch(f"{tag}_mat_{len(prog)}", 1, raw_x.h, raw_x.w, raw_x.c)
                prog.append(Step("apply", (raw_x, x[4], mode - 1, None, ms, None, 0)))   # apply modes: 0 norm, 1 norm + relu
            return x[4]

        def layer(x, pc, name, relu, res=None, defer=False):
            """-> relu?(norm(conv(x)))  or, with res,  relu(res + relu(norm(conv(x)))).
            x (and res) may be a PENDING activation ["raw", act, mode, stats, materialised]: a raw conv output whose
            InstanceNorm (+ ReLU) is deferred to its consumers -- fused into this conv's LDS-halo loader when this conv runs
            on that kernel, into the residual operand of the block's last normalisation kernel, materialised by the apply
            kernel otherwise.  defer=True returns such a pending activation."""
            xin, in_norm, in_stats = x, 0, None
            if isinstance(x, list):
                _, raw_x, mode, ms, mat = x
                if mat is None and ops.select_conv(raw_x, pc, in_norm=mode, precision=self.prec).in_norm:
                    xin, in_norm, in_stats = raw_x, mode, ms
                else:
                    xin = materialise(x)
            ho, wo = pc.out_hw(xin.h, xin.w)
            out = self._scratch(f"{tag}_{name}", 1, ho, wo, pc.cout)
            kw = dict(in_norm=in_norm, in_stats=in_stats) if in_norm else {}
            if not inorm:
                epi = EPI.EPI_RELU_RES_RELU if res is not None else (EPI.EPI_RELU if relu else EPI.EPI_LINEAR)
                prog.append(Step("conv", self._cp(xin, pc, out, epi=epi, e0=materialise(res) if res is not None else None, **kw)))
                return out
            raw = self._scratch(f"{tag}_raw_{name}", 1, ho, wo, pc.cout)
            p = self._cp(xin, pc, raw, stats=self.stats, **kw)
            rows = 2 * p._m_tiles
            ms = slot(name)
            prog.append(Step("conv", p))
            prog.append(Step("fin", (rows, pc.cout_pad, pc.cout, raw.cs, p._m, ms)))
            if defer and res is None:
                return ["raw", raw, 2 if relu else 1, ms, None]
            if res is None:
                prog.append(Step("apply", (raw, out, 1 if relu else 0, None, ms, None, 0)))
            elif isinstance(res, list) and res[4] is None:      # shortcut still raw: normalised inside this kernel
                prog.append(Step("apply", (raw, out, 2, res[1], ms, res[3], res[2])))
            else:
                prog.append(Step("apply", (raw, out, 2, materialise(res), ms, None, 0)))
            return out

        # conv1's output and the 1x1 downsample branch stay raw where every consumer can normalise on the fly (the LDS-halo
        # conv of the first block, the residual operand of a block's closing kernel): three apply passes fewer per encoder
        x = layer(img, e.conv1, "c1", True, defer=inorm and DEFER_NORM)
        for i, blk in enumerate(e.blocks):
            res = x if blk["stride"] == 1 else layer(x, blk["down"], f"b{i}_d", False, defer=inorm and DEFER_NORM)
            y = x
            for k, pc in enumerate(blk["convs"][:-1]):
                # the block-internal activations have exactly one consumer (the next conv of the block): their
                # normalisation is deferred to it (the block output is materialised)
                y = layer(y, pc, f"b{i}_{k}", True, defer=inorm)
            x = layer(y, blk["convs"][-1], f"b{i}_o", True, res=res)
        x = materialise(x)
        for pc, out, co_off, epi in outputs:
            prog.append(Step("conv", self._cp(x, pc, out, co_off=co_off, epi=epi)))
        return prog

    def _volume_program(self):
        sp = self.eng.spec
        prog = []
        alpha = 1.0 / math.sqrt(float(sp.fdim))
        x3 = self.prec_corr == "bf16x3"
        if self.otf and self.prec != "fp32" and PYRAMID_ONE_LAUNCH and sp.fdim % 32 == 0 and self.f2act[0].cs == sp.fdim and sp.levels <= 4:
            # pooled maps and split operands of all levels in one launch (was 2 * levels - 1 launches)
            return [Step("pyramid", ops.PyramidArgs(self.f2act[:sp.levels], self.f2s[:sp.levels], 3 if x3 else 1))]
        for l in range(sp.levels):
            if l > 0:
                prog.append(Step("pool", (self.f2act[l - 1], self.f2act[l])))
            if self.otf:        # only the operands: pooled maps, split once (exact fp32: the maps themselves)
                if self.prec != "fp32":
                    prog.append(Step("split", (self.f2act[l].t, self.f2s[l])))
                continue
            prog.append(Step("tile", (self.f2act[l], self.f2rows[l])))
            if self.prec == "fp32":
                prog.append(Step("conv", ops.corr_volume(self.f1, self.f2rows[l], self.vol[l].shape[1], self.vol[l], alpha)))
            else:               # both operands pre-split once, GEMM fed by LDS-DMA (woft_corr_gemm_bf16)
                prog.append(Step("split", (self.f2rows[l], self.f2s[l])))
                prog.append(Step("cgemm", (self.f1s, self.f2s[l], self.P, self.vol[l].shape[1], alpha, self.vol[l],
                                       3 if x3 else 1)))
        return prog

    # ---- one refinement iteration (update.py:106-112,127-136; weighted_raft.py:228-237) ----
    def _iter_program(self, first):
        e, cp, sp = self.eng, self._cp, self.eng.spec
        hd = sp.hdim
        h_in = self.net0 if first else self.hB
        prog = [Step("lookup", self.lookup)]
        if sp.small:            # SmallMotionEncoder update.py:71-77: cor(96) | flo(32) -> 80, cat flow
            prog += [Step("conv", cp(self.corr, e.convc1, self.cf, co_off=0, epi=EPI.EPI_RELU)),
                     Step("conv", cp(self.flow4, e.convf1, self.fl1, epi=EPI.EPI_RELU)),
                     Step("conv", cp(self.fl1, e.convf2, self.cf, co_off=96, epi=EPI.EPI_RELU)),
                     Step("conv", cp(self.cf, e.convm, self.xbuf, co_off=sp.cdim, epi=EPI.EPI_RELU))]
        else:                   # BasicMotionEncoder update.py:89-97: cor(192) | flo(64) -> 126, cat flow
            flo = [Step("conv", cp(self.flow4, e.convf1, self.fl1, epi=EPI.EPI_RELU), "convf1"),
                   Step("conv", cp(self.fl1, e.convf2, self.cf, co_off=192, epi=EPI.EPI_RELU), "convf2")]
            cor = [Step("conv", cp(self.corr, e.convc1, self.c1, epi=EPI.EPI_RELU), "convc1"),
                   Step("conv", cp(self.c1, e.convc2, self.cf, co_off=0, epi=EPI.EPI_RELU), "convc2")]
            if PAIR_BRANCHES:
                for c_, f_ in zip(cor, flo):             # (larger layer first: its workgroups are dispatched first)
                    if ops.pair_ok(c_.arg, f_.arg):
                        prog.append(Step("conv2", (c_.arg, f_.arg), c_.tag + "+" + f_.tag))
                    else:
                        prog += [c_, f_]
            else:
                prog += cor + flo
            prog.append(Step("conv", cp(self.cf, e.convm, self.xbuf, co_off=sp.cdim, epi=EPI.EPI_RELU), "convm"))
        # GRU half steps on [h | motion] (the inp term is the per-pixel gate bias, see RaftEngine): z|r conv (sigmoid, r*h fused),
        # q conv (tanh + state blend fused)
        steps = len(e.zr_dyn)
        states = [h_in, self.hA, self.hB] if steps == 2 else [h_in, self.hB]
        if steps == 1 and not first:
            states = [self.hB, self.hA]          # single-step GRU: ping-pong hB -> hA, copied back below
        for k in range(steps):
            hi, ho = states[k], states[k + 1]
            gz, gq = self.gate_bias[k]
            pzr = cp(hi, e.zr_dyn[k], self.zbuf, x2=self.xbuf, x2_off=sp.cdim, c_split=hd,
                     epi=EPI.EPI_GRU_ZR, split=hd, e0=hi, out1=self.rh, bias_map=gz)
            pq = cp(self.rh, e.q_dyn[k], ho, x2=self.xbuf, x2_off=sp.cdim, c_split=hd,
                    epi=EPI.EPI_GRU_Q, e0=hi, e1=self.zbuf, bias_map=gq)
            prog += [Step("conv", pzr, f"gru_zr{k}"), Step("conv", pq, f"gru_q{k}")]
        if steps == 1 and not first:
            prog.append(Step("copy", (self.hA.t, self.hB.t)))
        fused = None
        if e.fh2_frag is not None and e.fh2.cout == 2:
            if self.fh_part is None:
                self.fh_part = torch.zeros(4 * self.P, 20, dtype=torch.float32, device="cuda")
            fused = ops.flowhead_params(self.hB, e.fh1, self.fh_part, e.fh2_frag, precision=self.prec)
        if fused is not None:                            # conv1 with conv2's partial products in its epilogue + the gather
            prog += [Step("conv", fused, "fh1"), Step("fh_gather", (fused._n_planes, e.fh2.bias[:2].contiguous()))]
            return prog
        prog.append(Step("conv", cp(self.hB, e.fh1, self.fh, epi=EPI.EPI_RELU), "fh1"))
        if ops.narrow_ok(self.fh, e.fh2):                # second conv + coords1 += delta in one launch
            prog.append(Step("fh_update", (self.fh, e.fh2, self.delta)))
        else:
            prog += [Step("conv", cp(self.fh, e.fh2, self.delta)), Step("coords", None)]
        return prog

    # ---- execution ------------------------------------------------------------------------
    def run(self, prog):
        ev = self.conv_events
        fused = False
        for k, (kind, a, tag) in enumerate(prog):
            if fused:                                        # (convc1 [+ convf1]: ran with the lookup before it)
                fused = False
                continue
            if kind == "conv":                               # (ev, a bench hook: HIP events around the launches whose tag it names)
                ops.run_conv(a) if ev is None else _timed(ev.get(tag), ops.run_conv, a)
            elif kind == "conv2":
                ops.run_conv_pair(*a) if ev is None else _timed(ev.get(tag), ops.run_conv_pair, *a)
            elif kind == "fin":
                rows, ld, c, c_pad, count, ms = a
                ops.inorm_finalize(self.stats, rows, ld, c, count, ms[0], ms[1], channels_pad=c_pad, ws=self.fin_ws)
            elif kind == "apply":
                raw, out, mode, res, ms, res_ms, res_mode = a
                ops.inorm_apply(raw, ms[0], ms[1], out, mode, res=res, res_stats=res_ms, res_mode=res_mode)
            elif kind == "pyramid":
                ops.feature_pyramid(a)
            elif kind == "pool":
                ops.avgpool2(a[0], a[1])
            elif kind == "split":
                self._split(a[0], a[1])
            elif kind == "tile":
                ops.tile_rows(a[0], a[1])
            elif kind == "cgemm":
                ops.corr_gemm_bf16(*a)
            elif kind == "lookup":
                fused = k + 1 < len(prog) and self._c1_on_band(a, prog[k + 1])
                if fused:
                    self._lookup_c1_band(a, prog[k + 1])
                else:
                    self._lookup(a)
            elif kind == "copy":
                a[1].copy_(a[0])
            elif kind == "fh_gather":
                ops.flow_head_gather(self.fh_part, a[0], self.hf, self.wf, a[1], self.delta, self.coords, self.flow4.t,
                                     self.flow_cat, self.xbuf.cs)
            elif kind == "fh_update":
                ops.flow_head_update(a[0], a[1], a[2], self.coords, self.flow4.t, self.flow_cat, self.xbuf.cs)
            elif kind == "coords":
                ops.coords_update(self.coords, self.delta.t, self.delta.cs, self.wf, self.flow4.t, self.flow_cat, self.xbuf.cs)
            else:
                raise ValueError(kind)

    def _lookup(self, params):
        if self.band_valid:
            _timed(self.lookup_events, self._lookup_band, params)
            return
        _timed(self.lookup_events, ops.run_lookup_otf if self.otf else ops.run_lookup, params)

    # ---- correlation band ------------------------------------------------------------------
    def band_applies(self, lookups, has_init=False):
        """Whether a flow of `lookups` lookups (iterations, + 1 with a weight head) runs on the correlation band: volume-free
        correlation in a split-bf16 mode, a (radius, k) the band kernels are built for, no warm start (the band is centred on
        the identity), and -- corr_band = "auto" -- enough lookups for the build to pay."""
        e, sp = self.eng, self.eng.spec
        if not CORR_BAND or e.corr_band is False or not self.otf or self.prec == "fp32" or has_init:
            return False
        if (sp.radius, sp.fdim) not in ops.BAND_INSTANCES or sp.levels > 4:
            return False
        return e.corr_band is True or lookups >= BAND_MIN_LOOKUPS

    def _band_buffers(self):
        if self._band is None:
            sp = self.eng.spec
            rows = ops.band_geometry(sp.radius, sp.levels)[3]
            i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
            self._band = (torch.zeros(self.P * rows * ops.BAND_LD, dtype=torch.float32, device="cuda"), i32(self.P), i32(1))
        return self._band

    def _band_build(self):
        """The band of the current source and target operands (after the pyramid): one launch; resets the miss counter."""
        band, miss, count = self._band_buffers()
        count.zero_()
        ops.run_band_build(self._band_variant(self.lookup))
        self.band_valid = True

    def _band_variant(self, params):
        """The band lookup's struct for a volume-free lookup struct (kept per struct; its `need` is copied at every use), with the
        fallback's: the same launch with need = the miss flags and no folded gather."""
        key = id(params)
        if key not in self._band_params:
            band, miss, count = self._band_buffers()
            fb = ops.copy_params(params)
            fb.fh_part, fb.need = None, _lib.ptr(miss)
            fb._keep = (getattr(params, "_keep", None), miss)
            self._band_params[key] = (params, ops.make_lookup_band_params(params, band, miss, count), fb)
        _, bp, fb = self._band_params[key]
        bp.need = params.need
        bp._fallback = fb
        return bp

    def _lookup_band(self, params):
        """Band lookup, then the volume-free lookup on the blocks it flagged as missed (its other blocks return at once)."""
        bp = self._band_variant(params)
        ops.run_lookup_band(bp)
        ops.run_lookup_otf(bp._fallback)

    def _c1_on_band(self, params, nxt):
        """Whether the lookup `params` and the step after it run as the fused form: a valid band, whole-map launches (a
        restricted iteration keeps its three launches: the fused kernel takes no rectangle), and the step is convc1 -- alone or
        paired with convf1 -- of the instance woft_conv1x1_band is built for."""
        if not (self._fuse_c1 and self.band_valid) or nxt.tag not in ("convc1+convf1", "convc1"):
            return False
        sp = self.eng.spec
        c1 = nxt.arg[0] if nxt.kind == "conv2" else nxt.arg
        rect = lambda q: (q.roi_y0 | q.roi_x0 | q.roi_h | q.roi_w) != 0
        if params.need or rect(params) or (params.smp_y0 | params.smp_x0 | params.smp_h | params.smp_w) != 0 or rect(c1):
            return False
        return ((sp.radius, sp.fdim, sp.levels) == (4, 256, 4) and Kernel(c1.halo) is Kernel.GEMM_1X1
                and c1.precision in (1, 2, 3) and (c1.cin_pad, c1.cout_pad) == (352, 256)
                and c1.in0 == params.out and c1.cs0 == params.ldo)

    def _lookup_c1_band(self, params, nxt):
        """Band lookup with the samples deferred, the fallback on the blocks it flagged, then convc1 sampling the band itself
        (+ convf1 on the workgroups behind).  The lookup buffer keeps stale rows where blocks hit: nothing reads it before the
        next lookup (the final lookup, which feeds the weight head, is never followed by convc1)."""
        bp = self._band_variant(params)

        def lookup():
            bp.defer_samples = 1
            try:
                ops.run_lookup_band(bp)
            finally:
                bp.defer_samples = 0
            ops.run_lookup_otf(bp._fallback)
        _timed(self.lookup_events, lookup)
        c1, f1 = nxt.arg if nxt.kind == "conv2" else (nxt.arg, None)
        ev = self.conv_events
        _timed(None if ev is None else ev.get(nxt.tag), ops.run_conv1x1_band, c1, f1, bp)

    @property
    def band_miss_blocks(self):
        """8 x 8 blocks that missed the band since it was last built (reads the device counter: tools and tests only)."""
        return 0 if self._band is None else int(self._band[2].item())

    def _split(self, rows, out):
        """fp32 rows -> the correlation GEMM's bf16 operand: [hi | lo] lines (bf16x3) or the bf16 plane (bf16)."""
        if self.prec_corr == "bf16x3":
            ops.split_bf16_lines(rows, out)
        else:
            ops.split_bf16(rows, out, None)

    # ---- what the operand buffers hold ---------------------------------------------------------------
    # (every method that overwrites operands says so through these two: nothing else writes the owners or clears band_valid)
    def _source_changed(self, owner=None):
        """img[0] / fmap1 and its correlation operand, net, inp, the gate biases are being overwritten: `owner`'s from now on."""
        self.source_owner = owner
        self._operands_changed()

    def _target_changed(self, owner=None):
        """img[1] / the target maps are being overwritten: the image is `owner`'s, the maps nobody's until flow() has run."""
        self.target_owner, self.target_valid = owner, False
        self._operands_changed()

    def _operands_changed(self):
        self.band_valid = False                              # (no band is the new operands')

    @property
    def source_tag(self):
        return None if self.source_owner is None else self.source_owner[0]

    def load_image(self, slot, img_u8, pad_top, pad_left, owner=None):
        """img_u8 -> img[slot] (0: the source image, 1: the target image).  owner (target only): the caller's token for the
        image -- after the flow() that encodes it, `target_valid and target_owner == owner` says the target features are its."""
        if slot == 0:
            self._source_changed()
        else:
            self._target_changed(owner)
        ops.preprocess(img_u8, self.img[slot], self.hp, self.wp, pad_top, pad_left)

    def encode_source(self, reuse_target=False, owner=None):
        """fmap1, net, inp of the source image in img[0] (cacheable across frames: `source_owner == owner` for as long as nothing
        overwrote them; owner = (tag, key), None = nobody asks).
        reuse_target: the source image IS the target image of this plan's previous flow() (consecutive lost frames: frame t was the
        target of the t-1 -> t flow and is the source of the t -> t+1 flow, TRK:181-184) -- its feature map is this plan's level-0
        target map: copied (fp32 map + correlation operand, two device copies) instead of a second fnet pass over the same image by
        the same launch program (bit-identical).  Volume-free correlation only (the volume mode keeps the target operand in
        4x4-tile order); -> whether the features were reused."""
        reused = bool(reuse_target) and self.otf and self.target_valid
        self._source_changed(owner)
        if reused:
            self.f1rows[:self.P].copy_(self.f2act[0].t.view(self.P, -1))
            if self.prec != "fp32":
                self.f1s[:self.P].copy_(self.f2s[0])
        else:
            self.run(self.prog_f_src)
        self.run(self.prog_c_src)
        if self.prec != "fp32" and not reused:
            self._split(self.f1rows, self.f1s)
        self.inp_c.t.copy_(self.xbuf.t[:, :self.eng.spec.cdim])
        self.run(self.prog_gate_bias)
        return reused

    # ---- frame-features records: an image encoded once, restored as the source or target of any flow ----
    @property
    def record_dims(self):
        sp = self.eng.spec
        return sp.fdim, sp.hdim, sp.cdim

    def new_record(self):
        """An empty record for this plan's geometry: P * (fdim + hdim + cdim) floats of the caller's own."""
        return torch.empty(ops.features_record_floats(self.P, *self.record_dims), dtype=torch.float32, device="cuda")

    def encode_record(self, record):
        """fnet and cnet on the image in img[0] (the launch programs of encode_source), then the fnet map, net and inp packed into
        `record` (woft_features_pack).  Overwrites this plan's source maps: whatever source was resident here is gone, and the
        reuse book-keeping is reset (source_owner, target_owner, target_valid) -- the derived source state (split operand, gate
        biases) is NOT brought up to date, restore_source() does that."""
        self._source_changed()
        self._target_changed()
        self.run(self.prog_f_src)
        self.run(self.prog_c_src)
        ops.features_pack(self.f1rows, self.net0.t, self.xbuf.t, self.P, self.record_dims, record)

    def restore_source(self, record):
        """The state encode_source() leaves for the record's image, bit for bit, without an encoder pass: one unpack launch writes
        the fnet rows, net, inp (GRU input buffer and inp_c) and, where the correlation operand is [hi | lo] lines, those in the
        same pass (pad rows beyond P are never written: they stay zero); then the derived steps encode_source() runs -- the
        split where it is not fused, the gate-bias convs."""
        x3 = self.prec != "fp32" and self.prec_corr == "bf16x3"
        self._source_changed()
        ops.features_unpack(record, self.P, self.record_dims, self.f1rows, self.f1s if x3 else None, self.net0.t, self.xbuf.t,
                            self.inp_c.t)
        if self.prec != "fp32" and not x3:
            self._split(self.f1rows, self.f1s)
        self.run(self.prog_gate_bias)

    def restore_target(self, record):
        """The record's fnet map -> the level-0 target map f2act[0]: flow(target_restored=True) then skips prog_f_dst and derives
        the pyramid / volumes from it (prog_volume starts from f2act[0] in every corr mode).  Until that flow has run the level-0
        operand is stale: target_valid is cleared, flow() sets it."""
        self._target_changed()
        ops.features_unpack(record, self.P, self.record_dims, self.f2act[0].t)

    def set_flow_init(self, flow_init):
        """Copy the caller's initial flow -- (2, hf, wf), 1/8-resolution pixels of the padded image, any float dtype, either
        device -- into the plan's own buffer; flow(..., flow_init=True) then starts from it."""
        if tuple(flow_init.shape) != (2, self.hf, self.wf):
            raise ValueError(f"flow_init must have shape (2, {self.hf}, {self.wf}) for a {self.hp} x {self.wp} padded input, "
                             f"got {tuple(flow_init.shape)}")
        self.flow_init.copy_(flow_init, non_blocking=True)

    def flow_low(self):
        """The final coords1 - coords0 of the last flow() as a new (2, hf, wf) tensor (the reference network's flow_low,
        weighted_raft.py:240-255), read from flow4 -- what the last coordinate update wrote."""
        return self.flow4.t[:, :2].t().reshape(2, self.hf, self.wf).contiguous()

    def flow(self, iters, crop, h, w, flow_up=None, dst=None, wout=None, do_sigmoid=False, trace=None, defer_wh=False,
             mout=None, mask_sigmoid=False, flow_init=None, skip_wh=False, target_restored=False, graph=False):
        """Target features -> volume -> `iters` refinements -> full-resolution outputs.
        defer_wh (full weighted model with a weight region set): stop before the weight head -- flow_up / dst are final,
        wout is NOT written -- and let finish_weights() evaluate the head where the caller then says it reads the weights.
        mout (engine built with mask_head): receives the upsampled visibility-mask logits (h*w floats, cropped like wout, never
        passed through a sigmoid); the head runs after the weight head whether or not mout is given.
        mask_sigmoid (the tracker's visibility request only): mout receives the sigmoid of those logits instead -- the do_sigmoid
        flag the upsampling kernels already have for the weight channel.
        skip_wh (a caller that reads the flow only, e.g. the reverse flow of a forward-backward check): the weight head (and the
        mask head) are not evaluated and wout / mout are not written; flow_up / dst do not depend on either head.
        flow_init (weighted_raft.py:184,223-224: coords1 = coords1 + flow_init): None = start from zero flow; a (2, hf, wf)
        tensor = copied into the plan's buffer first (set_flow_init); True = the buffer as it stands.  The first iteration's
        motion encoder reads it as the flow, the later coordinate updates write coords1 - coords0 as ever.  With a trace, the
        trace is also called once as trace(plan, -1) after the initialisation, before the first iteration.
        target_restored: f2act[0] already holds the target's fnet map (restore_target): no encoder pass over img[1].
        graph: the launches (a static list on fixed buffers) as ONE hipGraph launch -- eager at the first sighting of a FlowKey,
        eager and then captured at the second, replayed from the third, leaving the plan's Python state as the captured flow
        left it; always eager under a trace or a bench event hook."""
        if iters < 1:
            raise ValueError("iters must be >= 1")
        if self._wh_train is not None:                       # (a weights_at() graph of an earlier flow in this plan is stale now: its
            self._wh_train["gen"] += 1                       #  backward would read this flow's upsampling mask -- it raises instead)
        if self._mh_train is not None:                       # (a visibility_at() / visibility_map() graph alike)
            self._mh_train["gen"] += 1
        if flow_init is not None and flow_init is not True:
            self.set_flow_init(flow_init)                    # (a captured graph reads the plan's buffer: the copy stays outside)
        # restricted iterations (set_flow_region): not under a trace (it reads whole maps) nor a warm start (flow_low is read everywhere)
        region = self.flow_region if (trace is None and flow_init is None) else None
        if region is not None and region["key"][1] != iters:
            region = None
        launch = lambda: self._flow(iters, crop, h, w, flow_up, dst, wout, do_sigmoid, trace, defer_wh, mout, mask_sigmoid,
                                    flow_init is not None, skip_wh, target_restored, region)
        if not graph or trace is not None or any(ev is not None for ev in (self.lookup_events, self.wh_events, self.conv_events)):
            return launch()
        key = FlowKey(iters, crop, h, w, _lib.ptr(flow_up), _lib.ptr(dst), _lib.ptr(wout), _lib.ptr(mout), bool(do_sigmoid),
                      bool(mask_sigmoid), bool(defer_wh), bool(skip_wh), flow_init is not None, bool(target_restored),
                      _lib.ptr(self.wh_region[0]) if self.wh_region is not None else None, region["key"] if region is not None else None)
        g = self._graphs.get(key)
        if g is not None:
            g.replay()
            self.band_valid, self.target_valid = g.post
            return
        launch()                                             # this call's results; also the warm-up the capture needs
        if key in self._graphs:                              # (second sighting: capture for the calls to come)
            g = _FlowGraph()
            with torch.cuda.graph(g):
                launch()
            g.post = (self.band_valid, self.target_valid)
        self._graphs[key] = g

    def _flow(self, iters, crop, h, w, flow_up, dst, wout, do_sigmoid, trace, defer_wh, mout, mask_sigmoid, has_init, skip_wh,
              target_restored, region):
        """The launches of flow() (has_init: from the plan's flow_init buffer; region: the restricted programs, or None)."""
        e, sp = self.eng, self.eng.spec
        self._fuse_c1 = FUSE_C1 and e.fuse_c1 and trace is None    # (a trace reads the lookup buffer after every iteration)
        self._target_changed(self.target_owner)              # (the maps become those of the image or record already put in place)
        if not target_restored:
            self.run(self.prog_f_dst)
        self.run(self.prog_volume)
        self.target_valid = True                             # (level-0 target map + operand now belong to the image in img[1])
        if self.band_applies(iters + (1 if e.weighted and not skip_wh else 0), has_init):
            self._band_build()
        if not has_init:
            ops.coords_init(self.coords, self.hf, self.wf, self.flow4.t, self.flow_cat, self.xbuf.cs)
        else:
            ops.coords_init_flow(self.coords, self.flow_init, self.hf, self.wf, self.flow4.t, self.flow_cat, self.xbuf.cs)
            if trace is not None:
                trace(self, -1)
        folded = self.folded is not None and trace is None   # (a trace reads the coordinates after every iteration)
        for it in range(iters):
            prog = self._iteration(it, iters, folded)
            self.run(prog if region is None else region["iters"].get(it, prog))
            if trace is not None:
                trace(self, it)
        if folded:
            self.run(self.folded.gather)
        # (the merged last iteration ran the upsampling-mask head's first conv with the flow head's)
        for p in self.prog_mask[1 if iters > 1 and self.prog_iter_last is not None else 0:]:
            ops.run_conv(p)
        if defer_wh or skip_wh:
            assert not defer_wh or (e.weighted and not sp.small and self.wh_region is not None and not e.mask_head)
            self._upsample(None, crop, h, w, flow_up=flow_up, dst=dst, wout=None, do_sigmoid=do_sigmoid)
            return
        if e.weighted:
            index, prog = self.wh_region if self.wh_region is not None else (None, self.prog_wh)
            self._weight_head(prog, index)
        wout = wout if e.weighted else None
        self._upsample(self.wlow, crop, h, w, flow_up=flow_up, dst=dst, wout=wout, do_sigmoid=do_sigmoid)
        if e.mask_head:
            self._mask_head()
            if mout is not None:        # the weight channel of the same upsampling kernels, on the mask logits (weighted_raft.py:305-308)
                self._upsample(self.mh_low, crop, h, w, wout=mout, do_sigmoid=mask_sigmoid)

    def _upsample(self, wlow, crop, h, w, **outputs):
        """Flow (and the 1/8-resolution map wlow) to full resolution: convex x8, or bilinear x8 on the small model, which has no
        upsampling mask (utils.py:82-84)."""
        if self.eng.spec.small:
            ops.upflow8(self.coords, wlow, self.hf, self.wf, crop, h, w, **outputs)
        else:
            ops.convex_upsample(self.coords, wlow, self.mask.t, self.hf, self.wf, crop, h, w, **outputs)

    def _mask_head(self):
        """MaskHead on the final coordinates (weighted_raft.py:295-304, 411-422) -> self.mh_low (1/8-resolution logits)."""
        e = self.eng
        ops.warp_features(self.f2act[0], self.coords, self.mh_warped)
        for p in self.prog_mh:
            ops.run_conv(p)
        ops.wh_reduce(self.mh_last, 1, self.mh_w, e.mh_b, self.P, self.mh_low)

    def finish_weights(self, pts, count, n_max, pad, crop, h, w, flow_up=None, dst=None, wout=None, do_sigmoid=False,
                       w_points=None):
        """After flow(defer_wh=True): the weight head on the windows of the current region that the (count) full-resolution
        pixels pts (n_max, 2) need (woft_wh_needed: the 3x3 upsampling support of their 1/8-res cells), then the upsampling
        with the weights.  wout is exact at those pixels (the head has no cross-pixel terms); elsewhere it is unspecified.
        w_points (n_max floats): receive the weights of the named pixels only, in their order, instead of the full map.
        pad = (top, left) of the padded image the 1/8-res grid belongs to."""
        index, _ = self.wh_region[:2]
        key = index.data_ptr()
        if key not in self._wh_dyn:
            dyn = torch.full_like(index, -1)
            prog, fused = self._wh_program(int(index.numel()), dyn)
            assert fused
            self._wh_dyn[key] = (dyn, prog, torch.zeros(self.P, dtype=torch.int32, device=index.device),
                                 torch.zeros(1, dtype=torch.int32, device=index.device))
        dyn, prog, bitmap, n_needed = self._wh_dyn[key]
        ops.wh_needed(pts, count, n_max, pad[0], pad[1], self.hf, self.wf, index, bitmap, dyn, n_needed)
        self._weight_head(prog, dyn, n_needed, need=bitmap)
        if w_points is not None:     # the weights of the named pixels only, in their order (no second full-resolution pass)
            ops.convex_weights_at(pts, count, n_max, self.wlow, self.mask.t, self.hf, self.wf, crop, w_points,
                                  do_sigmoid=do_sigmoid)
            return
        self._upsample(self.wlow, crop, h, w, flow_up=flow_up, dst=dst, wout=wout, do_sigmoid=do_sigmoid)

    def refresh_weight_head(self):
        """After RaftEngine.repack_weight_head: this plan's own copies -- wh0_t, the closing bias tensor, the padded closing weights
        -- refreshed in place, and no captured graph (a captured launch bakes the closing bias in as an argument)."""
        e = self.eng
        self.wh0_t.copy_(e.wh0.wgt[:128].t())
        self.wh6_b.fill_(e.wh6_b)
        if self._wh6_pad is not None:
            self._wh6_pad[:e.wh6_c].copy_(e.wh6_w[:e.wh6_c])
        self._graphs.clear()

    def _wh6_padded(self, cs):
        """The closing 1x1 conv's weights padded with zeros to the activation's channel stride (woft_wh_reduce walks whole rows)."""
        if self._wh6_pad is None or self._wh6_pad.numel() != cs:
            self._wh6_pad = torch.zeros(cs, dtype=torch.float32, device="cuda")
            self._wh6_pad[:self.eng.wh6_c] = self.eng.wh6_w[:self.eng.wh6_c]
        return self._wh6_pad

    def _head_input(self, need, x8):
        """What the weight head reads: the final lookup (weighted_raft.py:266; with `need`, on the volume-free lookup, only the 8x8
        blocks that hold a wanted window) -> corr, then the mean response -> wmean and, with x8, the packed patches."""
        sp = self.eng.spec
        if self.otf:
            self.lookup.need = _lib.ptr(need)
        self._lookup(self.lookup)
        if self.otf:
            self.lookup.need = None
        ops.colsum(self.f2act[0].t, self.P, sp.fdim, self.cs_ws, self.cs_tot)
        ops.wh_pack(self.corr, self.f1, self.cs_tot, 1.0 / (math.sqrt(float(sp.fdim)) * self.P), sp.nwin, self.wmean, x8)

    def _weight_head(self, prog_wh, index, n_needed=None, need=None):
        """Final lookup + the weight head (weighted_raft.py:266-272, 347-384) on all source pixels (index None) or on the
        windows listed in `index` -> self.wlow."""
        e, n = self.eng, self.eng.spec.nwin
        self._head_input(need, None if self.wh0_direct else self.x8)
        if self.x32 is not None:
            self.x32.t[:, :8].copy_(self.x8.t)                   # (generic head, first kernel wider than 3)
        n_win = int(index.numel()) if index is not None else self.P
        if index is not None:
            self.wlow.zero_()                                    # pixels outside the region
        if self.wh0_direct and not self.wh0_fused:
            ops.wh_conv0(self.corr, self.wmean, n_win, n, self.wh0_t, e.wh0.bias, self.a1, index)
        # bench hook: HIP events around the first 128->128 layer (dynamic window list: the number of windows that really ran is
        # on the device)
        _timed(self.wh_events, ops.run_conv, prog_wh[0], extra=lambda: n_win if n_needed is None else n_needed.clone())
        for p in prog_wh[1:]:
            ops.run_conv(p)
        if not self.wh_fused:
            last = self.a1 if e.wh_std else self.wh_last
            ops.wh_reduce(last, n * n, self._wh6_padded(last.cs), e.wh6_b, self.P, self.wlow)

    # ---- training of the weight head (woft_amd/wh_train.py) ------------------------------------------
    def _wh_train_buffers(self, n_max):
        """Buffers of the training path, sized by 9 * n_max windows (the 3x3 upsampling support of n_max points), allocated at
        the first use and again when a larger n_max arrives.  None of them is read by flow() / finish_weights()."""
        cap = 9 * n_max
        t = self._wh_train
        if t is None or t["cap"] < cap:
            z, P = self._z, self.P
            i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
            t = dict(cap=cap, x8=z(cap, 81, 8), act=[z(cap, 81, 128) for _ in range(3)], g=[z(cap, 81, 128) for _ in range(2)],
                     out=z(cap), wlow=z(P), g_wlow=z(P), bitmap=i32(P), dyn=i32(P),
                     all=torch.arange(P, dtype=torch.int32, device="cuda"),
                     ws=z(ops.wh_wgrad_ws_floats(cap, 128)), ws64=z(-(-cap // ops.WH_TRAIN_CHUNK) * 129, dtype=torch.float64),
                     gen=0 if t is None else t["gen"])
            self._wh_train = t
        return t

    def wh_train_forward(self, params, pts, count, n_max, pad, crop, do_sigmoid=False):
        """The weight of the last flow() at the (count) pixels pts (n_max, 2) = (x, y), by an un-fused exact-fp32 forward of the
        standard head that keeps its three activations: the windows the points need (woft_wh_needed) compacted into a list,
        the final lookup on their 8x8 blocks, mean response, the packed patches, three woft_wh_train_conv layers, the closing
        conv + window mean, woft_convex_weights_at.  params: the eight tensors of the head in state-dict order (net.0.weight,
        net.0.bias, ... net.6.bias), fp32 on the device, read as they are now.
        -> (wsel (n_max,) with exact zeros at and beyond count, state for wh_train_backward)."""
        sp, n = self.eng.spec, self.eng.spec.nwin
        assert self.eng.weighted and self.eng.wh_std and not sp.small and n == 9 and 0 < n_max <= ops.HFIT_SINGLE_MAX
        t = self._wh_train_buffers(n_max)
        t["gen"] += 1
        w0, b0, w2, b2, w4, b4, w6, b6 = (p.detach() for p in params)
        wsel = torch.zeros(n_max, dtype=torch.float32, device="cuda")
        ops.wh_needed(pts, count, n_max, pad[0], pad[1], self.hf, self.wf, t["all"], t["bitmap"], t["dyn"])
        index = t["dyn"][t["dyn"] >= 0].contiguous()     # (reads its length back: training has no per-frame latency budget)
        n_win = int(index.numel())
        if n_win == 0:
            return wsel, None
        self._head_input(t["bitmap"], None)
        li = index.long()
        x8 = t["x8"][:n_win]                             # woft_wh_pack's rows of the listed windows (channels 5..7 stay zero)
        x8[:, :, :4] = self.corr.t[li, :4 * n * n].view(n_win, n * n, 4)
        x8[:, :, 4] = self.wmean[li][:, None]
        wh_train.head_forward(x8, n_win, (w0, b0, w2, b2, w4, b4, w6), t["act"], t["out"])
        t["wlow"].zero_()
        t["wlow"][li] = t["out"][:n_win] + b6.reshape(())
        ops.convex_weights_at(pts, count, n_max, t["wlow"], self.mask.t, self.hf, self.wf, crop, wsel, do_sigmoid=do_sigmoid)
        return wsel, dict(gen=t["gen"], index=index, n_win=n_win, pts=pts, count=count, n_max=n_max, crop=crop,
                          do_sigmoid=bool(do_sigmoid), w2=w2.clone(), w4=w4.clone(), w6=w6.reshape(-1).clone())

    def wh_train_backward(self, state, g_wsel):
        """Gradients of the eight head parameters for the gradient g_wsel (n_max,) of wh_train_forward's result: upsampling
        adjoint -> closing conv + mean -> per layer the weight gradient (woft_wh_wgrad) and, above the first layer, the data
        gradient (woft_wh_train_conv with the transposed, flipped filter and the ReLU gate).  Reads the activations the forward
        left in the plan's training buffers and the plan's upsampling mask: it must run before the next wh_train_forward or
        flow() of this plan.  Deterministic: two calls return equal bytes."""
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
        gw0, gb0, gw2, gb2, gw4, gb4, gw6, gb6 = z(128, 5, 3, 3), z(128), z(128, 128, 3, 3), z(128), z(128, 128, 3, 3), z(128), \
            z(1, 128, 1, 1), z(1)
        grads = (gw0, gb0, gw2, gb2, gw4, gb4, gw6, gb6)
        if state is None:
            return grads
        t = self._wh_train
        if t is None or t["gen"] != state["gen"]:
            raise RuntimeError("weights_at(): backward after a later flow or weights_at() in the same flow plan -- the activations "
                               "and the upsampling mask it reads are gone")
        n_win, index = state["n_win"], state["index"]
        ops.convex_weights_at_bwd(state["pts"], state["count"], state["n_max"], g_wsel, t["wlow"], self.mask.t, self.hf, self.wf,
                                  state["crop"], t["g_wlow"], index=index, do_sigmoid=state["do_sigmoid"])
        wh_train.head_backward(t["x8"], n_win, (state["w2"], state["w4"], state["w6"]), t["act"], t["g_wlow"], index, t["g"],
                               t["ws"], t["ws64"], grads)
        return grads

    # ---- training of the mask head (woft_amd/mh_train.py) --------------------------------------------
    def refresh_mask_head(self):
        """After RaftEngine.repack_mask_head: this plan's own copy of the closing conv's weights refreshed in place, and no
        captured graph (a captured launch bakes the closing bias in as an argument)."""
        self.mh_w[:self.eng.mh_c].copy_(self.eng.mh_wlast)
        self._graphs.clear()

    def _mh_train_buffers(self):
        """Buffers of the training path, sized by the map (P pixels) and the head, allocated at the first use: one activation
        map per layer, two gradient maps as wide as the widest layer, the 1/8-resolution logits and their gradient, the partial
        sums of the widest weight gradient (ceil(hf * ceil(wf / 32) / 16) partials of 9 * C * cin + C floats) and of the closing
        conv (ceil(P / 256) * 129 doubles), the 9 P partial sums of the dense upsampling adjoint.  None of them is read by flow()."""
        t = self._mh_train
        if t is None:
            z, P, hf, wf = self._z, self.P, self.hf, self.wf
            shapes = self.eng.mh_shapes[:-1]
            t = dict(act=[z(P, s[0]) for s in shapes], g=[z(P, max(s[0] for s in shapes)) for _ in range(2)], out=z(P), low=z(P),
                     g_low=z(P), ws=z(max(ops.mh_wgrad_ws_floats(hf, wf, s[1], s[0]) for s in shapes)),
                     ws64=z(-(-P // ops.MH_REDUCE_CHUNK) * 129, dtype=torch.float64),
                     up=z(ops.convex_upsample_bwd_ws_floats(hf, wf)), gen=0)
            self._mh_train = t
        return t

    def _mh_head_forward(self, params):
        """The head part both training forwards share: a new generation of the training buffers, the exact-fp32 head on
        [fmap1 | mh_warped] into t["act"], t["out"] and, with the closing bias, t["low"] -> (t, the detached parameters)."""
        e = self.eng
        assert e.mask_head and not e.spec.small and mh_train.refusal(e.mh_shapes) is None
        t = self._mh_train_buffers()
        t["gen"] += 1
        ps = [p.detach() for p in params]
        mh_train.head_forward(self.f1rows, self.mh_warped.t, self.hf, self.wf, ps[:-1], t["act"], t["out"])
        torch.add(t["out"], ps[-1].reshape(()), out=t["low"])
        return t, ps

    def _mh_live(self, state, what):
        """The training buffers if they still hold the forward that made `state`, else the stale-graph error."""
        t = self._mh_train
        if t is None or t["gen"] != state["gen"]:
            raise RuntimeError(f"{what}(): backward after a later flow, visibility_at() or visibility_map() in the same flow plan "
                               "-- the activations and the upsampling mask it reads are gone")
        return t

    def mh_train_forward(self, params, pts, count, n_max, crop, do_sigmoid=False):
        """The visibility of the last flow() at the (count) pixels pts (n_max, 2) = (x, y), by an exact-fp32 forward of the
        MaskHead that keeps its activations: woft_mh_train_conv layers over the whole map on [fmap1 | mh_warped] (the warped target
        features that flow left), the closing conv, woft_convex_weights_at on the logits.  params: the head's tensors in state-dict
        order (net.0.weight, net.0.bias, ...), fp32 on the device, read as they are now.
        -> (vsel (n_max,) with exact zeros at and beyond count, state for mh_train_backward)."""
        assert 0 < n_max <= ops.HFIT_SINGLE_MAX
        t, ps = self._mh_head_forward(params)
        vsel = torch.zeros(n_max, dtype=torch.float32, device="cuda")
        ops.convex_weights_at(pts, count, n_max, t["low"], self.mask.t, self.hf, self.wf, crop, vsel, do_sigmoid=do_sigmoid)
        return vsel, dict(gen=t["gen"], pts=pts, count=count, n_max=n_max, crop=crop, do_sigmoid=bool(do_sigmoid),
                          shapes=[tuple(p.shape) for p in ps], w=[p.clone() for p in ps[2::2]])

    def mh_train_backward(self, state, g_vsel):
        """Gradients of the head's parameters for the gradient g_vsel (n_max,) of mh_train_forward's result: upsampling adjoint ->
        closing conv -> per layer the weight gradient (woft_mh_wgrad) and, above the first layer, the data gradient
        (woft_mh_train_conv with the transposed, flipped filter and the ReLU gate).  Reads the activations the forward left in the
        plan's training buffers, fmap1, mh_warped and the upsampling mask: it must run before the next mh_train_forward or flow() of
        this plan.  Deterministic: two calls return equal bytes."""
        t = self._mh_live(state, "visibility_at")
        grads = tuple(torch.zeros(s, dtype=torch.float32, device="cuda") for s in state["shapes"])
        ops.convex_weights_at_bwd(state["pts"], state["count"], state["n_max"], g_vsel, t["low"], self.mask.t, self.hf, self.wf,
                                  state["crop"], t["g_low"], do_sigmoid=state["do_sigmoid"])
        mh_train.head_backward(self.f1rows, self.mh_warped.t, self.hf, self.wf, state["w"], t["act"], t["g_low"], t["g"], t["ws"],
                               t["ws64"], grads)
        return grads

    def mh_dense_forward(self, params, crop, h, w, do_sigmoid=False):
        """The visibility of the last flow() at every pixel of the (h, w) crop window: the head as in mh_train_forward, then the
        inference path's own woft_convex_upsample on the logits (its weight output alone) -- at a pixel the bytes mh_train_forward
        returns there.  -> (map (h, w), a fresh tensor; state for mh_dense_backward)."""
        t, ps = self._mh_head_forward(params)
        out = torch.empty(h, w, dtype=torch.float32, device="cuda")
        ops.convex_upsample(self.coords, t["low"], self.mask.t, self.hf, self.wf, crop, h, w, wout=out, do_sigmoid=do_sigmoid)
        return out, dict(gen=t["gen"], crop=crop, size=(h, w), do_sigmoid=bool(do_sigmoid), shapes=[tuple(p.shape) for p in ps],
                         w=[p.clone() for p in ps[2::2]])

    def mh_dense_backward(self, state, g_map):
        """Gradients of the head's parameters for the gradient g_map (h, w) of mh_dense_forward's result: the dense upsampling
        adjoint (woft_convex_upsample_bwd: the mask read once, 9 P partials) -> t["g_low"], then mh_train_backward's head part.  The
        same conditions: before the next training forward or flow() of this plan; two calls return equal bytes."""
        t = self._mh_live(state, "visibility_map")
        grads = tuple(torch.zeros(s, dtype=torch.float32, device="cuda") for s in state["shapes"])
        h, w = state["size"]
        ops.convex_upsample_bwd(g_map, self.mask.t, t["low"], self.hf, self.wf, state["crop"], h, w, t["up"], t["g_low"],
                                do_sigmoid=state["do_sigmoid"])
        mh_train.head_backward(self.f1rows, self.mh_warped.t, self.hf, self.wf, state["w"], t["act"], t["g_low"], t["g"], t["ws"],
                               t["ws64"], grads)
        return grads
