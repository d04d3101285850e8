"""Flow-provider operator: the MI355X counterpart of the reference's RAFTWrapper
(/root/reference/pytracking/optical_flow/raft.py:29-218), same constructor config keys, same
`compute_flow` signature, return types and error behaviour.  `pytracking.optical_flow.raft`
(the compatibility shim) re-exports it under the reference's import path.
"""
import logging
import os
from collections import OrderedDict
from pathlib import Path
from timeit import default_timer as timer

import numpy as np
import torch

from . import _lib, mh_train, ops, wh_train
from .config import config_get
from .engine import RaftEngine

logger = logging.getLogger(__name__)


def _pad_geometry(h, w, mode):
    """-> (hp, wp, pad_top, pad_left, out_h, out_w, load_h, load_w)"""
    if mode == "nopad":                                   # raft.py:221-226
        assert h % 8 == 0
        assert w % 8 == 0
        return h, w, 0, 0, h, w, h, w
    if mode == "crop":                                    # raft.py:235-247 (outputs keep the cropped size)
        ch, cw = (h // 8) * 8, (w // 8) * 8
        return ch, cw, 0, 0, ch, cw, ch, cw
    if mode == "RAFT":                                    # raft_core/utils/utils.py:7-26, 'sintel' mode
        ph = (((h // 8) + 1) * 8 - h) % 8
        pw = (((w // 8) + 1) * 8 - w) % 8
        return h + ph, w + pw, ph // 2, pw // 2, h, w, h, w
    if mode == "Michal":
        # the reference's MichalPadder.unpad(None) raises AttributeError for raft_type 'orig' / 'weighted'
        # (raft.py:148-150,264-265): the mode is unreachable in every shipped configuration
        raise NotImplementedError("padding_mode 'Michal' (raft.py:250-271) fails in the reference itself for "
                                  "raft_type 'orig'/'weighted'; it is not provided on the HIP path")
    raise ValueError(f"invalid padding_mode '{mode}'")


def _mask_head_shapes(structure, fdim):
    """class_params.mask_head_structure -> the state-dict shapes of mask_head.net.{0,2,...}.weight (weighted_raft.py:387-409:
    (channels, kernel) tuples or plain channel counts = 3x3 layers, on 2 * fdim input channels; closing 1x1 conv to 1)."""
    try:
        layers = [tuple(d) if isinstance(d, (list, tuple)) else (d, 3) for d in structure]
        shapes, cur = [], 2 * fdim
        for c, k in layers:
            c, k = int(c), int(k)
            if c < 1 or k < 1 or k % 2 == 0:
                raise ValueError
            shapes.append((c, cur, k, k))
            cur = c
    except (TypeError, ValueError):
        raise ValueError(f"class_params.mask_head_structure {structure!r}: not a list of (channels, odd kernel) tuples "
                         "or channel counts (weighted_raft.py:387-409)") from None
    return shapes + [(1, cur, 1, 1)]


class FrameFeatures:
    """One frame, encoded: what RAFTWrapper.encode_frame() returns and compute_flow() accepts in place of
    an image, as source or as target.  Owns its device record -- the fnet map, net and inp in fp32, `nbytes` = 4 * P * (fdim +
    hdim + cdim): 66.4 MB for a 1080p frame on the full model -- never a view of a plan buffer; valid for the provider that made it,
    at the padded geometry it was made at, for as long as it is referenced (sync_weight_head() does not touch it: the encoders
    are frozen).
    provider; geometry = (hp, wp, top, left) of the padded image; size = (H, W) of the un-padded image; shape = (H, W, 3)."""

    def __init__(self, provider, record, geometry, size):
        self.provider, self.record = provider, record
        self.geometry, self.size = tuple(int(v) for v in geometry), tuple(int(v) for v in size)

    @property
    def shape(self):
        return self.size + (3,)

    @property
    def nbytes(self):
        return self.record.numel() * self.record.element_size()

    def __repr__(self):
        return f"FrameFeatures({self.size[0]} x {self.size[1]}, padded geometry {self.geometry}, {self.nbytes} bytes)"


class _Recent:
    """Least-recently-used book-keeping of RAFTWrapper.bound_plans(): touch(key, keep) marks `key` as used now and returns the
    keys that fall out -- all but the `keep` most recent ones, never the protected key (the one last touched with protect=True)."""

    def __init__(self):
        self.order, self.protected = OrderedDict(), None

    def touch(self, key, keep, protect=False):
        if protect:
            self.protected = key
        self.order[key] = None
        self.order.move_to_end(key)
        others = [k for k in self.order if k != self.protected]
        dropped = others[:max(0, len(others) - keep)]
        for k in dropped:
            del self.order[k]
        return dropped


class _LastFlow:
    """What the last compute_flow() of a provider left for the calls that follow it; a new one per call and per cache hit."""

    def __init__(self, low_plan=None):
        self.low_plan = low_plan   # flow_low(): the plan of the last COMPUTED flow (a cache hit since then leaves it)
        self.wh = None             # weights_at(): (plan, crop) of this call's computed flow
        self.size = None           # visibility_map(): (H, W) of that flow's un-padded outputs
        self.flow_map = None       # flow_map(): the (2, H, W) buffer this call wrote, if it wrote one
        self.deferred = None       # finish_weights(): (plan, crop, oh, ow, outputs, do_sigmoid) while weights are deferred


class RAFTWrapper:
    def __init__(self, config):
        self.C = config
        cp = config.class_params
        if self.C.raft_type not in ("orig", "weighted", "weighted_masked"):
            raise ValueError(f"Unknown RAFT type {self.C.raft_type}")
        # 'weighted_masked' (raft.py:38-42,142-147): WeightedRAFT with its MaskHead -> a visibility-mask output as well.  The two
        # keys must agree: the reference unpacks 6 network outputs for 'weighted_masked' and 5 for 'weighted' and fails at the
        # first flow with a ValueError when they do not -- here the same error class, at construction.  ('orig' ignores the key,
        # as the reference does: plain RAFT has no head.)
        self.masked = self.C.raft_type == "weighted_masked"
        if self.masked and not cp.mask_estimation:
            raise ValueError("raft_type 'weighted_masked' needs class_params.mask_estimation = True (and mask_head_structure): "
                             "without the MaskHead the network has no mask output")
        if self.C.raft_type == "weighted" and cp.mask_estimation:
            raise ValueError("class_params.mask_estimation is set with raft_type 'weighted', which returns no mask: use raft_type "
                             "'weighted_masked'")
        self._cache_mask_warned = False
        logger.info(f"Loading weights from: {self.C.model}")

        def read(src):
            sd = src if isinstance(src, dict) else torch.load(src, map_location="cpu")
            return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        state_dict = read(self.C.model)
        if self.C.backbone_model:
            # raft.py:58-62 drops every fnet / cnet / update_block tensor of `model` ("will overwrite backbone later ...
            # weights pre-trained on standard RAFT"); the overwrite itself is not in the reference's wrapper (the backbone
            # stays at its random initialisation there).  Here the announced merge is carried out: the backbone tensors
            # come from the `backbone_model` checkpoint (a path or a state-dict), everything else (the weight head) from `model`.
            in_backbone = lambda k: ("fnet" in k) or ("cnet" in k) or ("update_block" in k)
            state_dict = {k: v for k, v in state_dict.items() if not in_backbone(k)}
            state_dict.update({k: v for k, v in read(self.C.backbone_model).items() if in_backbone(k)})
        weighted = self.C.raft_type in ("weighted", "weighted_masked")
        small = bool(cp.small)
        if self.masked:             # (checked against the checkpoint before any device work)
            if not cp.mask_head_structure:
                raise ValueError("raft_type 'weighted_masked' needs class_params.mask_head_structure (weighted_raft.py:387-409)")
            want = _mask_head_shapes(cp.mask_head_structure, 128 if small else 256)
            idx = sorted(int(k.split(".")[2]) for k in state_dict if k.startswith("mask_head.net.") and k.endswith(".weight"))
            got = [tuple(state_dict[f"mask_head.net.{i}.weight"].shape) for i in idx]
            if got != want or idx != list(range(0, 2 * len(want), 2)):
                raise ValueError(f"class_params.mask_head_structure {cp.mask_head_structure!r} expects mask_head.net layers {want}; "
                                 f"the checkpoint has {got} (at net.{idx})")
        # arithmetic of the convolutions / correlation products: "bf16x3" (split-bf16 operands, fp32 accumulation: fp32-EMULATING,
        # ~2^-16 relative per product; flow EPE <= 1e-4 px against the fp32 reference at 1080p, budget 1e-3 px), "fp32" (exact fp32
        # MFMA products, 4x slower), "bf16", "f16mx8", or "fp16".  `mixed_precision=True` selects "fp16" with the reference's scoping
        # (autocast = fp16 around fnet, cnet and the update block only, weighted_raft.py:204-219,233-234; correlation, weight head
        # and upsampling stay fp32-class).
        # A flow config WITHOUT the key (an unmodified reference config) gets "bf16x3" since round 5, not exact fp32: the reference
        # pins torch 1.8.1 (README.org:33), whose defaults on the GPUs of its time are torch.backends.cudnn.allow_tf32 = True AND
        # torch.backends.cuda.matmul.allow_tf32 = True (the PyTorch default from 1.7 to 1.11; the reference never touches either
        # flag) -- its own convolutions and its correlation matmul multiply 10-bit-mantissa TF32 operands on an A100.  bf16x3's
        # 16-bit products are 64x finer than that; exact fp32 stays one key away (precision = 'fp32' / WOFT_PRECISION=fp32) and is
        # timed in every bench line.
        for src, val in (("env WOFT_PRECISION", os.environ.get("WOFT_PRECISION")),
                         ("flow config key 'precision'", self.C.precision),
                         ("class_params.mixed_precision", "fp16" if cp.mixed_precision else None),
                         ("built-in default (no key in the flow config): fp32-emulating bf16x3 -- finer than the TF32 convolutions "
                          "the reference's torch 1.8.1 runs by default on Ampere; 'fp32' = exact products", "bf16x3")):
            if val:
                self.precision, self.precision_source = str(val), src
                break
        # What arithmetic the caller got, said out loud: SURVEY 8a reads "IEEE fp32 unless stated", so anything else is STATED here --
        # at WARNING level when nobody asked for it (the built-in default of a config without the key), at INFO level otherwise.
        note = (f"RAFT arithmetic: precision = '{self.precision}' (from: {self.precision_source}). "
                + ("This is the reference's arithmetic (exact IEEE fp32 products)." if self.precision == "fp32" else
                   "NOT the reference's IEEE-fp32 products: set precision = 'fp32' in the flow config (or WOFT_PRECISION=fp32) "
                   "for the reference's arithmetic (about 4x slower)."))
        logger.log(logging.WARNING if self.precision_source.startswith("built-in default") else logging.INFO, note)
        self.precision_note = note
        # correlation: "volume" (all-pairs volume + pyramid in HBM, corr.py:13-69) or "otf" (volume-free lookup, what
        # the reference's `alternate_corr` switch selects, corr.py:72-100).  Bit-identical results in every precision
        # (exact fp32 included: the lookup's fp32-MFMA instantiation), "otf" is faster and needs no P x P buffer: the default.
        self.corr = os.environ.get("WOFT_CORR") or getattr(self.C, "corr", None) or "otf"
        # flow config key `volume_storage` ("fp32" | "bf16"): element type of the correlation volume (corr = "volume")
        # flow config key `corr_band` ("auto" | True | False; env WOFT_CORR_BAND=0: off): the correlations around the identity
        # computed once per flow, the lookups sampling from them (engine.py: CORR_BAND) -- "auto": flows long enough for it to pay
        v = config_get(self.C, "corr_band", "auto")
        self.corr_band = v if v == "auto" else bool(v)
        # flow config key `fuse_c1` (default True; env WOFT_FUSE_C1=0: off): on a band flow convc1 samples the band inside its
        # own launch (engine.py: FUSE_C1)
        self.fuse_c1 = bool(config_get(self.C, "fuse_c1", True))
        self.engine = RaftEngine(state_dict, small=small, weighted=weighted, precision=self.precision, corr=self.corr,
                                 volume_storage=getattr(self.C, "volume_storage", None), mask_head=self.masked,
                                 corr_band=self.corr_band, fuse_c1=self.fuse_c1)
        # training of the weight head (weight_head_parameters / weights_at / sync_weight_head): the head's tensors as loaded, the
        # Parameters made of them at the first request
        self._wh_loaded = {k: v for k, v in state_dict.items() if k.startswith("weight_head.net.")}
        self._wh_params = None
        # training of the mask head (mask_head_parameters / visibility_at / sync_mask_head), alike
        self._mh_loaded = {k: v for k, v in state_dict.items() if k.startswith("mask_head.net.")}
        self._mh_params = None
        # restricted refinement iterations for callers that declare where they read the flow (pin_flow_region + flow_region=True)
        self.flow_region_on = bool(config_get(self.C, "flow_region", os.environ.get("WOFT_FLOW_REGION", "1") != "0"))
        # opt-in (flow config key `graph`, env WOFT_GRAPH=1): the ~330 launches of a flow -- a static list per
        # resolution, fixed buffers, no allocation -- are captured once into a hipGraph and replayed per frame
        self.use_graph = (os.environ.get("WOFT_GRAPH") or str(int(bool(getattr(self.C, "graph", False))))) == "1"
        self._pinned, self._pins = None, 0     # the pinned source image; how many pin_source() calls there have been
        self._wmask, self._wregion, self._all_pixels = None, {}, {}
        self._fmask, self._fregion = None, {}
        self.weights_deferred, self._last = False, _LastFlow()
        self.defer_min_ratio = 6           # defer_weights: region windows per named pixel from which deferring pays
        self._out = {}
        self._cache_errors = set()
        self.source_features_reused = False
        self._plan_bound = None
        self._recent_plans, self._recent_outs, self._recent_pixels = _Recent(), _Recent(), _Recent()

    def bound_plans(self, n_other):
        """Opt-in bound on what the provider keeps per input shape (default: everything, for ever -- a tracker sees one or two
        shapes).  After this call it keeps the shape of the flows from the pinned source, plus the `n_other` most recently used
        other (shape, buffer set) pairs; older plans, their output buffers and window lists are dropped (least recently used
        first) and rebuilt if the shape returns.  For callers whose input size changes from call to call: the window tracker's
        frame t-1 -> t flows run on a box that follows the object."""
        self._plan_bound = None if n_other is None else max(1, int(n_other))

    def _touch_plan(self, plan_key, out_key, n_pix, pinned_here):
        """Book-keeping of bound_plans(): plans are filed by PADDED size, output buffers by the un-padded size (several per plan),
        the all-pixels window lists by 1/8-resolution pixel count -- of each, the pinned source's entry and the most recently
        used others stay.  (What this call uses was just touched: it is never among the dropped.)"""
        n = self._plan_bound
        if n is None:
            return
        for key in self._recent_plans.touch(plan_key, n, protect=pinned_here):
            self.engine.drop_plan(key)
        for key in self._recent_outs.touch(out_key, n, protect=pinned_here):
            self._out.pop(key, None)
        for key in self._recent_pixels.touch(n_pix, n, protect=pinned_here):
            self._all_pixels.pop(key, None)

    def finish_weights(self, pts, count, n_max, out=None):
        """After compute_flow(..., defer_weights=True) with `weights_deferred` set: evaluate the weight head for the
        (count, a device int32; at most n_max) source pixels pts (n_max, 2) = (x, y) and return the (1, H*W) weight tensor
        (borrowed), exact at those pixels and unspecified elsewhere -- or, with out (n_max floats), just the weights of
        the named pixels, in their order.  The weights of a source pixel do not depend on the
        other pixels (weighted_raft.py:363-383), and the caller knows which correspondences it keeps before it needs
        their weights (TRK:287-312 + subsampler: decided by the flow alone)."""
        plan, crop, oh, ow, o, do_sigmoid = self._last.deferred
        self._last.deferred = None
        plan.finish_weights(pts, count, n_max, crop, crop, oh, ow, flow_up=o["flow"], dst=o["dst"], wout=o["w"],
                            do_sigmoid=do_sigmoid, w_points=out)
        return o["w"] if out is None else out

    @property
    def _wh_flow(self):
        return self._last.wh

    # ---- training of the weight head (woft_amd/wh_train.py) ----
    def _wh_trainable(self):
        """NotImplementedError, naming the reason, unless this provider is the one case the training path covers."""
        eng = self.engine
        why = (f"raft_type '{self.C.raft_type}' (only 'weighted' is covered)" if self.C.raft_type != "weighted" else
               "the small model (its head reads 7x7 windows of another lookup)" if eng.small else
               "a weight_head_structure other than [(128, 3), (128, 3), (128, 3)]" if not eng.wh_std else
               "a weights_postprocessing_fn between the head and the weights" if self.C.weights_postprocessing_fn else None)
        if why:
            raise NotImplementedError(f"training of the weight head is not provided for {why}")

    def weight_head_parameters(self):
        """The weight head's parameters as an OrderedDict of fp32 device torch.nn.Parameter (requires_grad=True) under the
        reference's state-dict names weight_head.net.{0,2,4,6}.{weight,bias}, initialised from the loaded checkpoint; the same
        objects at every call.  weights_at() reads their current values; the inference path (compute_flow) reads its own packed
        copies, which sync_weight_head() refreshes.  torch.optim takes list(d.values()); dict(d) saves as a state dict."""
        self._wh_trainable()
        if self._wh_params is None:
            self._wh_params = wh_train.make_parameters(self._wh_loaded)
        return self._wh_params

    def weights_at(self, pts, count=None, do_sigmoid=False):
        """After a computed compute_flow(src, dst, ...) of this provider (skip_weights=True is the cheap way; not after a
        flow-cache hit): the flow weight at the pixels pts (n_max, 2) float32 = (x, y) of the un-padded source image (n_max <=
        2048), evaluated with the CURRENT values of weight_head_parameters() in exact fp32 -> (n_max,) float32, the logit or
        (do_sigmoid) its sigmoid; rows at and beyond count (a device int32 scalar, optional) are exact zeros.  With grad enabled
        and a parameter that requires grad the result carries a graph whose backward accumulates into the parameters' .grad
        (once differentiable; deterministic); nothing else receives a gradient -- RAFT stays frozen.  backward() must run before
        the next compute_flow / weights_at of this provider: it reads the plan's buffers."""
        self._wh_trainable()
        if self._last.wh is None:
            raise RuntimeError("weights_at(): no computed flow to evaluate the head on (none yet, or the last one came from the "
                               "flow cache)")
        if not (isinstance(pts, torch.Tensor) and pts.is_cuda and pts.dtype == torch.float32 and pts.dim() == 2
                and pts.shape[1] == 2 and pts.shape[0] >= 1):
            raise TypeError("weights_at(): pts must be a (n_max, 2) float32 device tensor of (x, y) pixels")
        if pts.shape[0] > ops.HFIT_SINGLE_MAX:
            raise ValueError(f"weights_at(): at most {ops.HFIT_SINGLE_MAX} points per call, got {pts.shape[0]}")
        if count is not None and not (isinstance(count, torch.Tensor) and count.is_cuda and count.dtype == torch.int32
                                      and count.numel() == 1):
            raise TypeError("weights_at(): count must be a device int32 scalar")
        plan, crop = self._last.wh
        params = self.weight_head_parameters().values()
        return wh_train.weights_at(plan, params, pts.detach().contiguous(), count, int(pts.shape[0]), crop, do_sigmoid)

    def sync_weight_head(self):
        """Push the current values of weight_head_parameters() into the inference path: every packed buffer the engine and its
        plans read head parameters from is rewritten in place and every captured graph is dropped.  Afterwards compute_flow
        returns the bits of a fresh provider built from the original state dict with dict(weight_head_parameters()) merged in."""
        self.engine.repack_weight_head({k: v.detach() for k, v in self.weight_head_parameters().items()})

    # ---- training of the mask head (woft_amd/mh_train.py) ----
    def _mh_trainable(self):
        """NotImplementedError, naming the reason, unless this provider is a case the training path covers."""
        eng = self.engine
        why = (f"raft_type '{self.C.raft_type}' (only 'weighted_masked' has a mask head)" if not self.masked else
               "the small model (no upsampling mask: its visibility is upsampled bilinearly)" if eng.small else
               mh_train.refusal(eng.mh_shapes))
        if why:
            raise NotImplementedError(f"training of the mask head is not provided for {why}")

    def mask_head_parameters(self):
        """The MaskHead's parameters as an OrderedDict of fp32 device torch.nn.Parameter (requires_grad=True) under the reference's
        state-dict names mask_head.net.{0,2,...}.{weight,bias}, initialised from the loaded checkpoint; the same objects at every
        call.  visibility_at() reads their current values; the inference path (compute_flow) reads its own packed copies, which
        sync_mask_head() refreshes.  torch.optim takes list(d.values()); dict(d) saves as a state dict."""
        self._mh_trainable()
        if self._mh_params is None:
            self._mh_params = mh_train.make_parameters(self._mh_loaded, self.engine.mh_shapes)
        return self._mh_params

    def visibility_at(self, pts, count=None, do_sigmoid=False):
        """After a computed compute_flow(src, dst, ...) of this provider (not after a flow-cache hit): the visibility logit at the
        pixels pts (n_max, 2) float32 = (x, y) of the un-padded source image (n_max <= 2048), evaluated with the CURRENT values
        of mask_head_parameters() in exact fp32, whatever the provider's precision -> (n_max,) float32, the logit or (do_sigmoid)
        its sigmoid; rows at and beyond count (a device int32 scalar, optional) are exact zeros.  With grad enabled and a
        parameter that requires grad the result carries a graph whose backward accumulates into the parameters' .grad (once
        differentiable; deterministic); nothing else receives a gradient -- fmap1, the warped fmap2, the upsampling mask and pts
        are frozen.  backward() must run before the next compute_flow / visibility_at of this provider: it reads the plan's
        buffers."""
        self._mh_trainable()
        if self._last.wh is None:
            raise RuntimeError("visibility_at(): no computed flow to evaluate the head on (none yet, or the last one came from "
                               "the flow cache)")
        if not (isinstance(pts, torch.Tensor) and pts.is_cuda and pts.dtype == torch.float32 and pts.dim() == 2
                and pts.shape[1] == 2 and pts.shape[0] >= 1):
            raise TypeError("visibility_at(): pts must be a (n_max, 2) float32 device tensor of (x, y) pixels")
        if pts.shape[0] > ops.HFIT_SINGLE_MAX:
            raise ValueError(f"visibility_at(): at most {ops.HFIT_SINGLE_MAX} points per call, got {pts.shape[0]}")
        if count is not None and not (isinstance(count, torch.Tensor) and count.is_cuda and count.dtype == torch.int32
                                      and count.numel() == 1):
            raise TypeError("visibility_at(): count must be a device int32 scalar")
        plan, crop = self._last.wh
        params = self.mask_head_parameters().values()
        return mh_train.visibility_at(plan, params, pts.detach().contiguous(), count, int(pts.shape[0]), crop, do_sigmoid)

    def visibility_map(self, do_sigmoid=False):
        """The dense form of visibility_at(), for supervision by a dense occlusion mask: after a computed compute_flow(src, dst,
        ...) of this provider (not after a flow-cache hit), the visibility logit -- or (do_sigmoid) its sigmoid -- at every pixel
        of the un-padded source image -> (H, W) float32 on the device, a fresh tensor; at a pixel it has the bytes visibility_at()
        returns there.  Evaluated with the CURRENT values of mask_head_parameters() in exact fp32, whatever the provider's
        precision.  With grad enabled and a parameter that requires grad the result carries a graph whose backward accumulates
        into the parameters' .grad (once differentiable; deterministic); nothing else receives a gradient.  backward() must run
        before the next compute_flow / visibility_at / visibility_map of this provider: it reads the plan's buffers."""
        self._mh_trainable()
        if self._last.wh is None:
            raise RuntimeError("visibility_map(): no computed flow to evaluate the head on (none yet, or the last one came from "
                               "the flow cache)")
        plan, crop = self._last.wh
        h, w = self._last.size
        return mh_train.visibility_map(plan, self.mask_head_parameters().values(), crop, h, w, do_sigmoid)

    def sync_mask_head(self):
        """Push the current values of mask_head_parameters() into the inference path: every packed buffer the engine and its plans
        read MaskHead parameters from is rewritten in place and every captured graph is dropped.  Afterwards compute_flow returns
        the bits of a fresh provider built from the original state dict with dict(mask_head_parameters()) merged in."""
        self.engine.repack_mask_head({k: v.detach() for k, v in self.mask_head_parameters().items()})

    # ---- template caching (results-identical: InstanceNorm is per sample, extractor.py:171-190) ----
    def pin_source(self, src_img):
        """Declare `src_img` (an ndarray the caller will not mutate) as a recurring source image:
        its feature/context tensors are computed once and reused by compute_flow(src_img, ...)."""
        self._pinned = src_img
        self._pins += 1                                    # (a source resident under an earlier pin is not this one's: see compute_flow)
        self._wmask, self._wregion = None, {}
        self._fmask, self._fregion = None, {}

    def pin_flow_region(self, mask):
        """Declare that, for flows FROM the pinned source image requested with flow_region=True, the caller reads the flow (and the
        weights) only at the pixels where `mask` (bool ndarray, source-image size; None = everywhere) is set.  The last refinement
        iterations then run only on the part of the 1/8-resolution map that the bounding rectangle of those pixels depends on
        (engine._Plan.set_flow_region): at the masked pixels flow, correspondences and weights are bit-identical, elsewhere they are
        unspecified but finite -- the contract finish_weights() has for the weights.  A mask that fills the frame restricts
        nothing and costs nothing."""
        self._fmask = None if mask is None else np.ascontiguousarray(np.asarray(mask) > 0)
        self._fregion = {}

    def _flow_region(self, key, hp, wp, top, left, oh, ow):
        """-> (y0, x0, h, w): the 1/8-resolution cells of the padded image that hold a pixel of the pinned flow mask, or None."""
        if self._fmask is None:
            return None
        if key not in self._fregion:
            ys, xs = np.nonzero(self._fmask[:oh, :ow])
            rect = None
            if ys.size:
                y0, y1, x0, x1 = (ys.min() + top) >> 3, (ys.max() + top) >> 3, (xs.min() + left) >> 3, (xs.max() + left) >> 3
                rect = (int(y0), int(x0), int(y1 - y0 + 1), int(x1 - x0 + 1))
            self._fregion[key] = rect
        return self._fregion[key]

    def pin_weight_region(self, mask):
        """Declare that, for flows FROM the pinned source image, the caller consumes the flow weights only at the
        pixels where `mask` (bool ndarray, source-image size; None = everywhere) is set: the weight head is then
        evaluated on those 1/8-resolution pixels only (+ the 3x3 support of the x8 upsampling), the other weights
        are unspecified.  The weights at the masked pixels are unchanged (the head is per source pixel,
        weighted_raft.py:363-383).  Flows from other sources always get the full weight map."""
        self._wmask = None if mask is None else np.ascontiguousarray(np.asarray(mask) > 0)
        self._wregion = {}

    def _weight_region(self, key, hp, wp, top, left, oh, ow):
        if self._wmask is None:
            return None
        if key not in self._wregion:
            m = self._wmask[:oh, :ow]
            coarse = np.zeros((hp // 8, wp // 8), bool)
            ys, xs = np.nonzero(m)
            coarse[(ys + top) >> 3, (xs + left) >> 3] = True
            pad = np.pad(coarse, 1)
            dil = np.zeros_like(coarse)
            for dy in range(3):                            # convex / bilinear x8 upsampling reads the 3x3 neighbours
                for dx in range(3):
                    dil |= pad[dy:dy + coarse.shape[0], dx:dx + coarse.shape[1]]
            idx = np.flatnonzero(dil).astype(np.int32)
            self._wregion[key] = torch.from_numpy(idx).cuda() if idx.size and idx.size < dil.size else None
        return self._wregion[key]

    def postprocess_weights(self, flat_weights, fn):
        s = self.last_flow_shape
        weights = fn(flat_weights.reshape(s["batch"], 1, s["H"], s["W"]))
        return weights.reshape(s["batch"], s["H"] * s["W"])

    def _outputs(self, h, w):
        key = (h, w)
        if key not in self._out:
            z = lambda *s: torch.empty(*s, dtype=torch.float32, device="cuda")
            self._out[key] = dict(flow=z(2, h, w), dst=z(2, h * w), w=z(1, h * w),
                                  src=torch.stack([torch.arange(h * w, device="cuda") % w,
                                                   torch.div(torch.arange(h * w, device="cuda"), w, rounding_mode="floor")]))
            if self.masked:
                self._out[key]["m"] = z(1, h * w)         # visibility-mask logits (weighted_masked)
        return self._out[key]

    def _cached_flow(self, src_img, identifier, mode, numpy_out, do_sigmoid, borrow=False):
        """utils/caching.py:53-59 wire format: <flow_cache_dir>/<dataset>/<sequence>/<i>-<i+1>.npz holding
        'half_flow' (2,H,W) and 'half_weights' (1,H,W) (any float dtype, cast to fp32); then the same
        post-processing as a computed flow (raft.py:152-195)."""
        dataset_name, seq_name, frame_i = identifier
        self._last = _LastFlow(self._last.low_plan)        # (a cache hit leaves the network's buffers at an older flow: weights_at() refuses)
        path = Path(self.C.flow_cache_dir) / dataset_name / seq_name / f"{frame_i}-{frame_i + 1}.npz"
        data = np.load(path, allow_pickle=False)           # plain float arrays: nothing to unpickle
        flow = np.ascontiguousarray(data["half_flow"].astype(np.float32))
        wts = data["half_weights"].astype(np.float32)
        wts = np.ascontiguousarray(wts) if wts.size > 1 else None
        h, w = flow.shape[1:]
        post = self.C.weights_postprocessing_fn if wts is not None else None
        o = self._outputs(h, w)
        o["flow"].copy_(torch.from_numpy(flow), non_blocking=True)
        wl = None
        if wts is not None:
            wl = torch.from_numpy(wts).cuda(non_blocking=True)
        lib = _lib.load()
        _lib.check(lib.woft_flow_to_tc(_lib.ptr(o["flow"]), _lib.ptr(wl), h, w, _lib.ptr(o["dst"]),
                                       _lib.ptr(o["w"]) if wl is not None else None, int(bool(do_sigmoid) and not post),
                                       _lib.stream_ptr()), "woft_flow_to_tc")
        if post:
            self._postprocess_logits(o, h, w, do_sigmoid)
        return self._deliver(o, o["w"] if wl is not None else None, mode, h, w, numpy_out, borrow)

    def _postprocess_logits(self, o, h, w, do_sigmoid):
        """raft.py:152-159: `weights_postprocessing_fn` maps the (1, 1, H, W) weight LOGITS, then the sigmoid (if asked)."""
        wts = self.C.weights_postprocessing_fn(o["w"].reshape(1, 1, h, w))
        wts = torch.as_tensor(wts, device=o["w"].device, dtype=torch.float32).reshape(1, h * w)
        o["w"].copy_(torch.sigmoid(wts) if do_sigmoid else wts)

    def _deliver(self, o, weights, mode, oh, ow, numpy_out, borrow):
        """The caller's view of the outputs.  The kernels write into per-resolution buffers that the NEXT call at the
        same size overwrites; like the reference, compute_flow hands out tensors of its own (device copies, a few
        microseconds) unless the caller passes borrow=True and consumes the results before its next call (the
        tracker does)."""
        own = (lambda t: t) if borrow else (lambda t: t.clone())
        host = lambda t: t.cpu().numpy()
        conv = host if numpy_out else own
        # weighted_masked (raft.py:170-173,180-181,201-203,215-216): the visibility-mask logits follow the weights -- (1, H, W) in
        # mode 'flow', (1, H*W) in mode 'TC' -- never through do_sigmoid / weights_postprocessing_fn (those act on the weights only)
        extra = ()
        if mode == "flow":
            wts = weights.reshape(1, oh, ow) if weights is not None else None
            if self.masked:
                extra = (conv(o["m"].reshape(1, oh, ow)),)
            return (conv(o["flow"]), (conv(wts) if wts is not None else None)) + extra
        self.last_flow_shape = {"batch": 1, "delta": 2, "H": oh, "W": ow}
        if self.masked:
            extra = (conv(o["m"]),)
        if numpy_out:
            return (host(o["src"]), host(o["dst"]), (host(weights) if weights is not None else None)) + extra
        # (the int64 source grid is a constant of the resolution -- 33 MB at 1080p: the provider's own tensor under borrow=True
        #  (the tracker only indexes it); any other caller gets a tensor it may edit in place, as the reference's callers may --
        #  round-4 advisor finding: a shared grid that a caller offsets or sorts would corrupt every later call at this size)
        return (own(o["src"]), own(o["dst"]), (own(weights) if weights is not None else None)) + extra

    @staticmethod
    def _as_flow_init(flow_init, hp, wp):
        """The caller's flow_init -> a float32 (2, hp/8, wp/8) torch tensor (its own device), or ValueError."""
        want = (2, hp // 8, wp // 8)
        t = flow_init if isinstance(flow_init, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(flow_init))
        if t.dim() == 4 and t.shape[0] == 1:
            t = t[0]
        if tuple(t.shape) != want or not t.is_floating_point():
            raise ValueError(f"flow_init must be a float array of shape {want} or {(1,) + want} (1/8-resolution pixels of the "
                             f"{hp} x {wp} padded image), got {tuple(flow_init.shape)} {flow_init.dtype}")
        return t.detach().to(torch.float32)

    def flow_key(self, src_img):
        """(buffer set, hp, wp, pad_top, pad_left) a compute_flow(src_img, ...) call would run in -- `last_flow_key` of a call
        that did: two flows with equal keys have 1/8-resolution grids of the same geometry (the tracker's warm start)."""
        hp, wp, top, left = _pad_geometry(src_img.shape[0], src_img.shape[1], self.C.padding_mode)[:4]
        return (0 if (src_img is self._pinned or self._pinned is None) else 1, hp, wp, top, left)

    def flow_low(self, copy=True):
        """After any COMPUTED flow (not a cache hit): its final 1/8-resolution flow coords1 - coords0, (2, hp/8, wp/8) fp32 on
        the device, in 1/8-resolution pixels of the padded image -- the reference network's flow_low (weighted_raft.py:240-255),
        which its wrapper drops.  copy=False: a view of the engine's buffer, valid until the next flow in the same buffer set."""
        plan = self._last.low_plan
        if plan is None:
            raise RuntimeError("flow_low(): no flow has been computed yet")
        return plan.flow_low() if copy else plan.flow4.t[:, :2].t().reshape(2, plan.hf, plan.wf)

    def flow_map(self):
        """After a computed compute_flow(mode='flow') or compute_flow(mode='TC', keep_flow=True): the (2, H, W) flow map of that
        call -- the provider's own buffer, valid until the next call at the same output size."""
        m = self._last.flow_map
        if m is None:
            raise RuntimeError("flow_map(): the last flow wrote no flow map (mode 'TC' without keep_flow, or no flow yet)")
        return m

    def _upload(self, a, H, W, lh, lw, what="compute_flow"):
        """An image argument -> its (lh, lw, 3) uint8 tensor on the device."""
        if isinstance(a, torch.Tensor):
            t = a if a.is_cuda else a.cuda(non_blocking=True)
        else:
            t = torch.from_numpy(np.ascontiguousarray(a)).cuda(non_blocking=True)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise TypeError(f"{what} takes (H, W, 3) uint8 BGR images, got {tuple(t.shape)} {t.dtype}")
        if (lh, lw) != (H, W):
            t = t[:lh, :lw].contiguous()
        return t.contiguous()

    def _operand_geometry(self, a):
        """(hp, wp, top, left, H, W) of an image or a FrameFeatures argument of compute_flow."""
        if isinstance(a, FrameFeatures):
            return a.geometry + a.size
        h, w = int(a.shape[0]), int(a.shape[1])
        return tuple(_pad_geometry(h, w, self.C.padding_mode)[:4]) + (h, w)

    def encode_frame(self, img):
        """Encode one frame once: img, (H, W, 3) uint8 BGR (numpy or a device tensor) -> FrameFeatures, which compute_flow() and
        compute_flow_fb() accept in place of the image, as source or target, any number of times; the flows have the bits of
        the flows from the image (InstanceNorm and eval-mode BatchNorm are per sample: the restored maps are the values the
        encoder passes of those flows would produce).  One fnet pass, one cnet pass and one pack launch; the record is a new
        device tensor of the caller's own (66.4 MB at 1080p on the full model).  Runs in the buffer set a flow from a non-pinned
        source runs in -- the pinned source's resident state is not touched -- and resets that set's reuse book-keeping
        (src_is_previous_dst finds nothing to reuse after it)."""
        H, W = img.shape[:2]
        hp, wp, top, left, oh, ow, lh, lw = _pad_geometry(H, W, self.C.padding_mode)
        slot = 0 if self._pinned is None else 1
        plan = self.engine.plan(hp, wp, slot)
        self._touch_plan((hp, wp) if slot == 0 else (hp, wp, slot), (oh, ow), plan.P, False)
        plan.load_image(0, self._upload(img, H, W, lh, lw, "encode_frame"), top, left)
        record = plan.new_record()
        plan.encode_record(record)
        return FrameFeatures(self, record, (hp, wp, top, left), (H, W))

    def compute_flow_fb(self, src_img, dst_img, alpha=0.01, beta=0.5, numpy_out=False, share_features=False):
        """Both flows of an image pair and their forward-backward consistency (no counterpart in raft.py)
        -> (flow_fwd (2, H, W), flow_bwd (2, H, W), err (1, H, W), ok (1, H, W)) as tensors of the caller's own (numpy_out: arrays).
        Two ordinary flows -- flow_fwd has the bits of compute_flow(src_img, dst_img, mode='flow'), flow_bwd those of
        compute_flow(dst_img, src_img, mode='flow') -- and one woft_flow_fb launch: with b = flow_bwd sampled at pixel + flow_fwd,
        err = |flow_fwd + b| and ok = 1.0 where that point is inside the frame and err^2 <= alpha * (|flow_fwd|^2 + |b|^2) + beta
        (else 0.0; outside the frame err = +inf).  Every raft_type and every padding_mode the provider has; the flow cache is not
        consulted.  Neither flow's weights are returned, so the weight head is skipped where the network allows it.
        Like any other call it replaces the state the previous call left (borrowed buffers, deferred weights, flow_low()).
        src_img / dst_img may be FrameFeatures.  share_features (default off): encode each image once (encode_frame) and run both
        directions from the records -- four encoder passes instead of six, the same bits."""
        alpha, beta = float(alpha), float(beta)
        if not (0.0 <= alpha < float("inf")) or not (0.0 <= beta < float("inf")):
            raise ValueError(f"compute_flow_fb: alpha and beta must be finite and >= 0, got {alpha!r}, {beta!r}")
        if share_features:
            src_img, dst_img = (a if isinstance(a, FrameFeatures) else self.encode_frame(a) for a in (src_img, dst_img))
        # (each flow is cloned out of the per-size output buffers before the next one overwrites them)
        fwd = self.compute_flow(src_img, dst_img, mode="flow", skip_weights=True)[0]
        bwd = self.compute_flow(dst_img, src_img, mode="flow", skip_weights=True)[0]
        err, ok = ops.flow_fb(fwd, bwd, alpha, beta)
        out = (fwd, bwd, err[None], ok[None])
        return tuple(t.cpu().numpy() for t in out) if numpy_out else out

    def compute_flow(self, src_img, dst_img, mode="TC", vis=False, src_img_identifier=None,
                     numpy_out=False, do_sigmoid=False, borrow=False, defer_weights=False, weight_region=False,
                     src_is_previous_dst=False, visibility=False, flow_init=None, iters=None, flow_region=False,
                     keep_flow=False, skip_weights=False):
        """src_img / dst_img: (H, W, 3) uint8 BGR (numpy, or CUDA tensors already on the device), or -- either or both -- the
        FrameFeatures that encode_frame() made of such an image: the flow then has the bits of the flow from the image, without
        the encoder passes over it.  A record must be this provider's and of the other operand's padded geometry, and cannot be
        combined with src_img_identifier (ValueError each).  A record as src is a non-pinned source: weight_region, defer_weights
        and flow_region are honoured or ignored exactly as for any non-pinned source image (flow_region and a pinned weight
        region: ignored; defer_weights with weight_region: honoured); src_is_previous_dst is ignored with it.  The pinned image as
        src with a record as dst keeps the pinned fast path and all three.
        mode 'TC' -> (src_coords (2,HW) int64, dst_coords (2,HW) f32, weights (1,HW) f32 | None)
        mode 'flow' -> (flow (2,H,W), weights (1,H,W) | None).
        raft_type 'weighted_masked' (raft.py:181,216): one more value, the visibility-mask logits -- (1,H,W) in mode 'flow',
        (1,HW) in mode 'TC' -- never passed through a sigmoid.
        borrow (extension, default off): return the provider's own output buffers, valid until the next call.
        weight_region (extension, default off): the caller reads the weights only inside the region declared with
        pin_weight_region() (flows from the pinned source); without it every call returns the full weight map, as the
        reference does.
        defer_weights (extension, default off: 0; else the number of source pixels the caller will name; honoured for flows
        from the pinned source whose weight region is large against it, else ignored: check `weights_deferred` after the
        call): return the flow / correspondences with weights = None and evaluate the weight head later, in
        finish_weights(), only where the caller then says it reads the weights.
        visibility (extension, default off; raft_type 'weighted_masked' only -- the tracker's visibility modes): the fourth value
        is the visibility PROBABILITY, the sigmoid of the mask logits (taken in the mask's upsampling call, the do_sigmoid flag of
        the weight channel), instead of the logits.
        flow_init (extension, default off: None; the reference NETWORK's argument, weighted_raft.py:184,223-224, which the reference's
        wrapper never passes): the refinement starts from coords1 = grid + flow_init instead of the identity grid.  (2, hp/8, wp/8)
        or (1, 2, hp/8, wp/8) -- 1/8-resolution pixels of the PADDED image (hp, wp), what the network receives -- as a torch
        tensor (either device) or a numpy float array; any other shape raises a ValueError that names the expected one.  Ignored
        on a flow-cache hit (the cache bypasses the network).  flow_low() after a call returns what the next call of a video
        would pass through woft_amd.warm.forward_interpolate.
        iters (extension, default None = the flow config's `iters`): the number of refinement iterations of THIS call.
        flow_region (extension, default off): the caller reads flow, correspondences and weights only inside the region declared
        with pin_flow_region() (flows from the pinned source, no flow_init, no visibility mask, no weights_postprocessing_fn; config
        key `flow_region` = False / env WOFT_FLOW_REGION=0 switch it off): identical values there, unspecified but finite ones
        elsewhere.  Without it every call computes the whole map, as the reference does.
        keep_flow (extension, default off): mode 'TC' writes the (2, H, W) flow map as well (the same upsampling launch; the
        correspondences are unchanged) and flow_map() hands it out, for a caller that needs both forms of one flow.
        skip_weights (extension, default off; ignored on a flow-cache hit): the caller reads the flow only -- weights come back as
        None and the weight head is not evaluated (the flow does not depend on it: bit-identical).  A 'weighted_masked' network
        evaluates both heads regardless (its mask output stays valid)."""
        if visibility and not self.masked:
            raise ValueError("compute_flow(visibility=True) needs raft_type 'weighted_masked': no other type has a mask output")
        assert mode in ["flow", "TC"]
        src_rec = src_img if isinstance(src_img, FrameFeatures) else None
        dst_rec = dst_img if isinstance(dst_img, FrameFeatures) else None
        if src_rec is not None or dst_rec is not None:
            for rec in (src_rec, dst_rec):
                if rec is not None and rec.provider is not self:
                    raise ValueError("compute_flow: a FrameFeatures record of another provider (its encoders made other features)")
            if src_img_identifier is not None:
                raise ValueError("compute_flow: src_img_identifier (the flow cache) cannot be combined with a FrameFeatures record")
            gs, gd = self._operand_geometry(src_img), self._operand_geometry(dst_img)
            if gs != gd:
                raise ValueError(f"compute_flow: the operands have different padded geometries (hp, wp, top, left, H, W): src {gs}, "
                                 f"dst {gd} -- a FrameFeatures record serves only the geometry it was encoded at")
        assert src_img.shape == dst_img.shape
        self._last = _LastFlow(self._last.low_plan)
        if src_img_identifier is not None and self.masked:
            # (deviation: the flow cache holds no mask -- utils/caching.py:53-59 -- and the reference raises UnboundLocalError on a
            #  cache hit with 'weighted_masked' (raft.py:171,202); here the cache is skipped and the flow computed, with its mask)
            if not self._cache_mask_warned:
                self._cache_mask_warned = True
                logger.warning("raft_type 'weighted_masked': the flow cache holds no visibility mask -- cached flows are not used, "
                               "every flow is computed")
        elif src_img_identifier is not None:               # pre-computed flow (raft.py:92-109)
            try:
                return self._cached_flow(src_img, src_img_identifier, mode, numpy_out, do_sigmoid, borrow)
            except Exception as ex:   # no such file / array, object placeholders, truncated archives, wrong shapes / dtypes:
                # the reference falls back on ANY exception (raft.py:108-109): compute the flow
                key = (type(ex), str(ex))                  # (the reference logs each distinct error once)
                if key not in self._cache_errors:
                    self._cache_errors.add(key)
                    logger.warning(f"no cached flow: {ex}")
        H, W = src_img.shape[:2]
        hp, wp, top, left, oh, ow, lh, lw = _pad_geometry(H, W, self.C.padding_mode)
        # a flow from another source leaves the pinned source's tensors (fmap1, net, inp, gate biases) where they are:
        # it runs in a second buffer set (the reference's lost branch, TRK:181-184, alternates template and frame t-1)
        pinned_here = src_img is self._pinned
        slot = 0 if (pinned_here or self._pinned is None) else 1
        plan = self.engine.plan(hp, wp, slot)
        if flow_init is not None:
            flow_init = self._as_flow_init(flow_init, hp, wp)
        n_iters = int(self.C.iters) if iters is None else int(iters)
        if n_iters < 1:
            raise ValueError("iters must be >= 1")
        self._touch_plan((hp, wp) if slot == 0 else (hp, wp, slot), (oh, ow), plan.P, pinned_here)
        start_time = timer()

        up = lambda a: self._upload(a, H, W, lh, lw)
        key = (hp, wp, top, left)
        # (the pinned source claims what encode_source() leaves; the plan drops the claim when anything overwrites that state)
        owner = (self, (self._pins,) + key) if pinned_here else None
        if owner is not None and plan.source_owner == owner:
            pass                                           # fmap1 / net / inp still resident in the plan
        elif src_rec is not None:                          # the source state of an encode_source() of the record's image
            plan.restore_source(src_rec.record)
            self.source_features_reused = False
        else:
            plan.load_image(0, up(src_img), top, left)
            # src_is_previous_dst (extension, the shim's tracker on consecutive lost frames): the caller states that src_img is the
            # image it passed as dst_img in its previous call for this buffer set; honoured only when that is the very same object
            # and geometry -- then the source features are the previous call's target features (engine.encode_source)
            reuse = bool(src_is_previous_dst) and plan.target_owner == (id(src_img), key)
            self.source_features_reused = bool(plan.encode_source(reuse_target=reuse, owner=owner))
        post = self.C.weights_postprocessing_fn or None     # (a map -> map callable may read any pixel: full map)
        region = None
        if weight_region and not post:
            if pinned_here:
                region = self._weight_region(key, hp, wp, top, left, oh, ow)
            if region is None and defer_weights:
                # no pinned region (another source, or no mask declared), but the caller will name the pixels whose weights
                # it reads (defer_weights): the window list is every source pixel, thinned on the device in finish_weights()
                if plan.P not in self._all_pixels:
                    self._all_pixels[plan.P] = torch.arange(plan.P, dtype=torch.int32, device="cuda")
                region = self._all_pixels[plan.P]
        plan.set_weight_region(region)
        frect = None
        if flow_region and self.flow_region_on and pinned_here and not post and flow_init is None and not self.masked:
            frect = self._flow_region(key, hp, wp, top, left, oh, ow)
        plan.set_flow_region(frect, n_iters)
        if dst_rec is not None:
            plan.restore_target(dst_rec.record)            # (img[1] is not this target: nothing for src_is_previous_dst to reuse)
        else:
            # (owner: what this buffer set's target features will belong to after this call)
            plan.load_image(1, up(dst_img), top, left, owner=(id(dst_img), key))
        o = self._outputs(oh, ow)
        weighted = self.C.raft_type in ("weighted", "weighted_masked") and not skip_weights
        # (defer_weights = the number of pixels the caller will name: worth it only if their 3x3 supports cannot cover most
        # of the region anyway -- measured with 500 pixels: +0.7 % at 720p (3 900 windows), +6 % at 1080p, +11 % at 4K)
        # (weighted_masked: the mask head has 3x3 cross-pixel terms and runs on every pixel after the weight head -- not deferred)
        self.weights_deferred = bool(defer_weights and weighted and not self.masked and not self.engine.small
                                     and plan.wh_region is not None
                                     and mode == "TC" and not numpy_out
                                     and int(plan.wh_region[0].numel()) > self.defer_min_ratio * int(defer_weights))
        self._last.wh, self._last.size = (plan, (top, left)), (oh, ow)
        self._last.deferred = (plan, (top, left), oh, ow, o, bool(do_sigmoid)) if self.weights_deferred else None
        want_flow = mode == "flow" or bool(keep_flow)      # (mode "TC" hands out dst = grid + flow only: no (2, H, W) flow map)
        plan.flow(n_iters, (top, left), oh, ow, flow_up=o["flow"] if want_flow else None, dst=o["dst"],
                  wout=o["w"] if weighted else None, do_sigmoid=bool(do_sigmoid) and not post, defer_wh=self.weights_deferred,
                  mout=o.get("m"), mask_sigmoid=bool(visibility), flow_init=flow_init, skip_wh=bool(skip_weights) and not self.masked,
                  target_restored=dst_rec is not None, graph=self.use_graph)
        self._last.flow_map = o["flow"] if want_flow else None
        self._last.low_plan, self.last_flow_key = plan, (slot,) + key
        if self.weights_deferred:
            return self._deliver(o, None, mode, oh, ow, numpy_out, borrow)
        logger.debug(f"flow enqueue time [s]: {float(timer() - start_time)}")
        weights = o["w"] if weighted else None
        if post and weights is not None:
            self._postprocess_logits(o, oh, ow, do_sigmoid)    # the logits, then the sigmoid (raft.py:152-159)
        return self._deliver(o, weights, mode, oh, ow, numpy_out, borrow)
