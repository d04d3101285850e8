"""WOFT tracker on the HIP flow / fit operators: the counterpart of the reference's
YAOFTrackerSingleControl (/root/reference/pytracking/tracker/YAOF_tracker_single_control.py,
TRK below) with the same constructor / init / track / set_fast_meta surface, the same config keys
and the same `meta` fields, so reference-style config files and WOFT_demo.py drive it unchanged.

Organisation (this file's own, not the reference's): a frame is `_global_stage` (template ->
pre-warped frame) and, when the re-detection test rejects its homography, `_local_stage`
(frame t-1 -> frame t); both hand a dense correspondence field plus the two masks that prune it
to ONE solver, `_solve`, which has two interchangeable back ends with identical results (tested
bit for bit):

  * device back end  -- configs built from woft_amd.presets (tagged callables): masking,
    order-preserving compaction, Sobol selection, H fit (least squares / IRLS, RANSAC, or the RANSAC
    similarity) and inlier test are HIP kernels (csrc/select.hip, csrc/hfit.hip, csrc/ransac.hip, csrc/trs.hip) with ONE
    device->host read per flow;
  * callable back end -- any other reference-format config: the keep rule runs as the same
    `select` kernel (woft_tc_flags), the surviving correspondences are handed to the config's own
    subsampler / estimator / re-detection callables exactly as TRK:141-162,196-199 hands them.

Visibility (this project's own, no counterpart in TRK; DESIGN.md "Visibility mask in the tracker"): with the config key
`visibility_mode` = 'gate' | 'weight' the flow config is a 'weighted_masked' one, and the MaskHead's per-pixel visibility probability
prunes ('gate': p > `visibility_thr`) or scales ('weight': w * p) the correspondences inside the same select kernels, in both stages
and both back ends.

Forward-backward check (this project's own, no counterpart in TRK): with the config key `fb_check` = 'gate'
both stages also run the REVERSE flow, compare the two (woft_flow_fb, keys `fb_alpha` / `fb_beta`) and hand the 0/1 verdict to the
solver in the visibility slot as a gate -- a reliability signal for networks that have none (raft_type 'orig').

Warm start (this project's own, no counterpart in TRK; DESIGN.md "Warm start"): with the config key `warm_start_local` the
frame t-1 -> t flow of the second and later frames of a run of lost frames starts from the forward-interpolated 1/8-resolution
flow of the previous one (RAFT's video warm start, raft_core/utils/utils.py:28-56) instead of from zero; `warm_start_iters`
sets the iteration count of those flows.  `meta.local_warm_started` says which kind a lost frame's flow was.

Photometric refinement (this project's own, no counterpart in TRK): with the config key `photo_refine` = N
the pose of every frame that is not lost is aligned to the frame's pixels by N Gauss-Newton iterations on the device
(woft_amd.photo) after the correspondence fit and before it becomes the tracker's pose; `meta.H_flow_cur2init` keeps the fit's
pose, `meta.photo` says what the refinement did.

Frames live on the GPU (the two cv2.warpPerspective calls of TRK:89-95 are one HIP kernel) and the
template's feature / context tensors are computed once (the flow provider pins the template).
"""
import logging
import os
from inspect import signature
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .config import config_get, config_set
from .homography import compose_H
from .planar import BoundedCache, PlanarBuffers, _Fit, decode, fit_and_judge

logger = logging.getLogger(__name__)
_EYE = np.eye(3)


def _count_components(mask_bool):
    from scipy import ndimage
    _, n = ndimage.label(mask_bool, structure=np.ones((3, 3), dtype=bool))   # 8-connected, as findContours
    return n


def make_forward_compatible(subsampler_fn):
    """Subsamplers written for (coords_a, coords_b, weights) are lifted to the 4-argument form that also carries the
    post-hoc weights (TRK:344-362); a lifted one cannot forward post-hoc weights and says so."""
    if len(signature(subsampler_fn).parameters) != 3:
        return subsampler_fn

    def lifted(coords_a, coords_b, weights, post_weights):
        if post_weights is not None:
            raise NotImplementedError("a 3-argument subsampler cannot carry post-hoc processed weights; "
                                      "give it a 4th parameter")
        return (*subsampler_fn(coords_a, coords_b, weights), None)
    if hasattr(subsampler_fn, "woft_spec"):
        lifted.woft_spec = subsampler_fn.woft_spec
    return lifted


def _device_u8(img, copy=False):
    """(H, W[, C]) uint8 image -> packed CUDA tensor (the kernels take raw pointers to packed uint8 rows)."""
    if isinstance(img, torch.Tensor):
        t = img if img.is_cuda else img.cuda()
    else:
        a = np.asarray(img)
        if a.dtype != np.uint8:
            raise TypeError(f"frames and masks must be uint8, got {a.dtype}")
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if t.dtype != torch.uint8:
        raise TypeError(f"frames and masks must be uint8, got {t.dtype}")
    if not t.is_contiguous():
        return t.contiguous()
    return t.clone() if copy and t is img else t


class _FrameUploader:
    """Host frames (numpy, as WOFT_demo.py:61-78 / TRK:113-120 hand them to track()) -> one of two alternating device buffers,
    so that the frame that becomes `prev_img` stays valid while the next one arrives (the local stage reads frame t-1,
    TRK:181-184).  Measured on the GPU box (tools/micro/upload_probe.py, 1080p BGR = 6.2 MB): the runtime's own pageable copy
    0.131 ms -- it pipelines its staging internally and sits at the PCIe floor (6.2 MB / ~55 GB/s = 0.11 ms) --; one memcpy into a
    pinned buffer + one asynchronous H2D copy 0.35 ms (round 4's path: the two do not overlap); the same in 4 pipelined pieces
    (woft_upload_u8) 0.18 ms, in 8 pieces 0.38 ms (a hipMemcpyAsync call costs ~20 us).  So the frame is copied DIRECTLY
    (`WOFT_UPLOAD=staged`: the pinned path in 4 pieces).  Nothing of a frame's GPU work can start before its pixels are there, and
    the caller hands over frame t only after frame t-1's result: the 0.13 ms are on the critical path (1.5 % of a 1080p frame).
    LIFETIME of what track() keeps: `tracker.prev_img` (and anything else holding the returned device frame) is valid until
    the SECOND next host-frame track() call, which reuses its buffer; a caller that wants a frame for longer clones it.  A change
    of frame shape allocates new buffers (the old prev_img stays valid, as its own tensor)."""
    STAGED = os.environ.get("WOFT_UPLOAD", "direct") == "staged"

    def __init__(self):
        self.key, self.stage, self.dev, self.done, self.i = None, None, None, None, 0

    def __call__(self, a):
        a = np.asarray(a)
        if a.dtype != np.uint8:
            raise TypeError(f"frames and masks must be uint8, got {a.dtype}")
        key = a.shape
        if key != self.key:
            self.dev = [torch.empty(key, dtype=torch.uint8, device="cuda") for _ in range(2)]
            if self.STAGED:
                self.stage = [torch.empty(key, dtype=torch.uint8).pin_memory() for _ in range(2)]
                self.done = [torch.cuda.Event(), torch.cuda.Event()]
            self.key, self.i = key, 0
        i = self.i = self.i ^ 1
        if not self.STAGED:
            self.dev[i].copy_(torch.from_numpy(np.ascontiguousarray(a)))       # (returns when the host pages have been read)
            return self.dev[i]
        self.done[i].synchronize()                   # (the copy that last read this staging buffer: two frames ago)
        if a.flags.c_contiguous and a.nbytes >= (1 << 20):
            from . import _lib
            _lib.check(_lib.load().woft_upload_u8(a.ctypes.data, self.stage[i].data_ptr(), self.dev[i].data_ptr(), a.nbytes, 4,
                                                  _lib.stream_ptr()), "woft_upload_u8")
        else:                                        # (non-contiguous views, e.g. a BGR<->RGB flipped array; small frames)
            np.copyto(self.stage[i].numpy(), a)
            self.dev[i].copy_(self.stage[i], non_blocking=True)
        self.done[i].record()
        return self.dev[i]


def _float_key(C, key, default, ok, what):
    """A config key as a float that satisfies ok() (NaN fails every compare), or ValueError naming `what` was expected."""
    v = config_get(C, key, default)
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{key} {v!r}: not {what}") from None
    if not ok(v):
        raise ValueError(f"{key} {v!r}: not {what}")
    return v


class YAOFTrackerSingleControl:
    DEVICE = "cuda"                  # (a host-logic test may build the tracker around a stub flow provider on "cpu")

    VISIBILITY_MODES = ("gate", "weight")
    # a 'weighted_masked' flow config is refused without a `visibility_mode` (nobody would read the mask); a subclass whose flows
    # are consumed elsewhere (woft_amd.chained.WOFTChained: the fold reads the mask) says so here
    MASK_NEEDS_VISIBILITY_MODE = True

    def _visibility_config(self):
        """-> (mode | None, threshold as the fp32 value the kernels compare with).  Config keys `visibility_mode` (absent / falsy:
        off) and `visibility_thr` (a float in (0, 1), default 0.5; read by 'gate' only)."""
        C = self.C
        mode = config_get(C, "visibility_mode")
        if not mode:
            return None, 0.5
        if mode not in self.VISIBILITY_MODES:
            raise ValueError(f"visibility_mode {mode!r}: not one of {self.VISIBILITY_MODES} (or absent / None: the mask is not used)")
        if C.flow_config.raft_type != "weighted_masked":
            raise ValueError(f"visibility_mode {mode!r} needs a flow config with raft_type 'weighted_masked' (the MaskHead computes the "
                             f"visibility); this one has {C.flow_config.raft_type!r}")
        thr = _float_key(C, "visibility_thr", 0.5, lambda v: 0.0 < v < 1.0, "a float in (0, 1)")
        return mode, float(np.float32(thr))                  # rounded to fp32 once, here

    FB_MODES = ("gate",)

    def _fb_config(self):
        """-> (mode | None, alpha, beta).  Config keys `fb_check` (absent / falsy: off; 'gate' is the only mode) and `fb_alpha` /
        `fb_beta` (finite floats >= 0, defaults 0.01 and 0.5): a correspondence survives iff its flow lands inside the frame and
        |f + b|^2 <= fb_alpha * (|f|^2 + |b|^2) + fb_beta, b the reverse flow sampled where f lands."""
        C = self.C
        mode = config_get(C, "fb_check")
        if not mode:
            return None, 0.01, 0.5
        if mode not in self.FB_MODES:
            raise ValueError(f"fb_check {mode!r}: not one of {self.FB_MODES} (or absent / None: no forward-backward check)")
        vm = config_get(C, "visibility_mode")
        if vm:
            raise ValueError(f"fb_check {mode!r} and visibility_mode {vm!r} are both set: the solver has one visibility slot, "
                             "choose one of the two")
        ok = lambda v: 0.0 <= v < float("inf")
        return (mode, _float_key(C, "fb_alpha", 0.01, ok, "a finite float >= 0"),
                _float_key(C, "fb_beta", 0.5, ok, "a finite float >= 0"))

    def _warm_start_config(self):
        """-> (on, iterations of a warm-started flow | None = the flow config's).  Config keys `warm_start_local` (absent / falsy:
        off) and `warm_start_iters` (an integer >= 1; absent / None: the flow config's `iters`)."""
        C = self.C
        on = config_set(C, "warm_start_local")
        n = config_get(C, "warm_start_iters")
        if n is not None and (isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1):
            raise ValueError(f"warm_start_iters {n!r}: not an integer >= 1")
        return on, (None if n is None else int(n))

    def _photo_config(self, ns=""):
        """-> None (off: `photo_refine` absent, None or 0) or the options of the photometric refinement (woft_amd.photo; DESIGN.md
        section 27): dict(iters, gain_bias, huber_k, min_valid, eps, stride, blur_sigma) from the config keys `photo_refine` (the
        iteration count), `photo_gain_bias` (True), `photo_huber_k` (None), `photo_min_valid` (0.5), `photo_eps` (1e-3),
        `photo_stride` (1), `photo_blur_sigma` (0).  ns: a prefix of every key (the chained trackers read `chain_photo_refine`, ...)."""
        C = self.C
        iters = config_get(C, f"{ns}photo_refine")
        if iters is None or (not isinstance(iters, bool) and isinstance(iters, (int, np.integer)) and iters == 0):
            return None
        from . import photo
        D = photo.DEFAULTS
        iters, gain_bias, huber_k, min_valid, eps = photo.check_options(
            iters, config_get(C, f"{ns}photo_gain_bias", D["gain_bias"]), config_get(C, f"{ns}photo_huber_k", D["huber_k"]),
            config_get(C, f"{ns}photo_min_valid", D["min_valid"]), config_get(C, f"{ns}photo_eps", D["eps"]),
            prefix=f"{ns}photo_refine / {ns}photo_")
        stride = config_get(C, f"{ns}photo_stride", 1)
        if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1:
            raise ValueError(f"{ns}photo_stride {stride!r}: not an integer >= 1")
        sigma = _float_key(C, f"{ns}photo_blur_sigma", 0.0, lambda v: 0.0 <= v < float("inf"), "a finite float >= 0")
        return dict(iters=iters, gain_bias=gain_bias, huber_k=huber_k, min_valid=min_valid, eps=eps, stride=int(stride),
                    blur_sigma=sigma)

    def _photo_options(self):
        """The keyword arguments of a refine() call."""
        P = self._photo
        return dict(iters=P["iters"], gain_bias=P["gain_bias"], huber_k=P["huber_k"], min_valid=P["min_valid"], eps=P["eps"])

    def _photo_decision(self, which):
        """The refinement's part of `solver_decision`."""
        P = self._photo
        return (f"; photometric refinement of {which} frames ({P['iters']} iterations, "
                + ("gain and bias" if P["gain_bias"] else "no gain / bias")
                + (f", Huber {P['huber_k']:.9g}" if P["huber_k"] is not None else "")
                + (f", stride {P['stride']}" if P["stride"] != 1 else "")
                + (f", blur {P['blur_sigma']:.9g}" if P["blur_sigma"] else "") + ")")

    def _photo_image(self, img):
        """The image the photometric stage reads: the uint8 device frame, or with `photo_blur_sigma` its blurred float32 version."""
        img = _device_u8(img)
        if not self._photo["blur_sigma"]:
            return img
        from . import hsynth
        return hsynth.augment(img, blur_sigma=self._photo["blur_sigma"], want_f32=True)[1]

    def _photo_stage(self, frame, H_cur2init, meta):
        """Align the fitted pose to the pixels: W0 = inv(H_cur2init) (template -> frame) refined against the template and its mask;
        -> inv(W), normalised as compose_H normalises.  meta.photo says what happened; a refinement without an eligible iterate
        returns the pose it was given."""
        if not np.all(np.isfinite(H_cur2init)):                      # (nothing to start from: the pose stays what the fit gave)
            meta.photo = None
            return H_cur2init
        W, info = self._photo_template.refine(self._photo_image(frame), np.linalg.inv(H_cur2init), **self._photo_options())
        self.host_wait_s += info.host_wait_s
        return self._photo_result(H_cur2init, W, info, meta)

    @staticmethod
    def _photo_result(H_cur2init, W, info, meta):
        """What a refinement returned -> meta.photo and the pose: inv(W), or the given pose when no iterate was eligible."""
        b = info.best
        meta.photo = SimpleNamespace(status=info.status, best=b, iterates=len(info.cost), rms_before=info.rms_before,
                                     rms_after=info.rms_after, n_valid=int(info.n_valid[b]) if b >= 0 else 0,
                                     gain=float(info.gain[b]) if b >= 0 else 1.0, bias=float(info.bias[b]) if b >= 0 else 0.0)
        if b < 0:
            return H_cur2init
        return compose_H(np.linalg.inv(W))

    # config keys this tracker class does not provide: (key, why), refused by __init__ when set
    REFUSED = ()
    REFUSED_BY = "tracker"
    BUFFER_SETS = 1                  # planar-stage buffer sets kept (a new grid size replaces the old one)

    def _refusals(self, config):
        for key, why in self.REFUSED:
            if config_set(config, key):
                raise NotImplementedError(f"{key} is not provided by the {self.REFUSED_BY}: {why}")

    def __init__(self, config):
        self._refusals(config)
        self.C = config
        self._photo = self._photo_config()    # (read once: None = off, and the frame's code path is what it is without the key)
        self._photo_template = None
        self.warm_start_local, self.warm_start_iters = self._warm_start_config()
        self.local_warm_started = False   # whether the last frame t-1 -> t flow started from a carried flow
        self._warm = None                 # (flow_low of the last frame t-1 -> t flow, its provider flow key): the carried flow
        self.fb_check, self.fb_alpha, self.fb_beta = self._fb_config()
        self.visibility_mode, self.visibility_thr = self._visibility_config()
        # what the solver's visibility slot carries: the MaskHead's probability under a visibility mode, the forward-backward
        # verdict (0 / 1, gated at 0.5) under fb_check -- never both (_fb_config)
        self._vis_mode, self._vis_thr = (("gate", 0.5) if self.fb_check else (self.visibility_mode, self.visibility_thr))
        if config.flow_config.raft_type == "weighted_masked" and self.visibility_mode is None and self.MASK_NEEDS_VISIBILITY_MODE:
            # the tracker unpacks (src, dst, weights) from compute_flow (TRK:101,181); a 'weighted_masked' provider returns a fourth
            # value, the visibility mask, which the tracker consumes only under a `visibility_mode`: refused here rather than at the first frame
            raise ValueError("the tracker takes a flow config with raft_type 'orig' or 'weighted'; 'weighted_masked' (MaskHead "
                             "visibility mask) returns a mask the tracker does not consume unless visibility_mode = 'gate' or "
                             "'weight' is set")
        if self.C.subsampler_fn:
            self.C.subsampler_fn = make_forward_compatible(self.C.subsampler_fn)
        self.flower = config.flow_config.of_class(config.flow_config)
        if self.fb_check and not (hasattr(self.flower, "flow_map") and hasattr(self.flower, "pin_source")):
            raise NotImplementedError("fb_check needs this project's flow provider (compute_flow(..., keep_flow=True) and "
                                      f"flow_map()); {type(self.flower).__name__} has neither")
        self.device = self.DEVICE
        self._fused = self._fused_specs()
        self._sparse_weights = False
        self.n_kept = None                # correspondences kept by the masks (and the gate) in the last solve
        self._replay = None
        self._announced = False
        self._local_chain = None          # (target frame object, frame number) of the last frame t-1 -> t flow
        self._n_tracked = 0
        self._upload = _FrameUploader()
        self.host_wait_s = 0.0       # seconds this tracker's thread spent blocked on the per-flow result read (device back end)
        self._buffers = BoundedCache(self.BUFFER_SETS)    # (K, grid size, cap) -> PlanarBuffers
        self._prewarp = BoundedCache()                    # frame / window shape -> (pre-warped frame, its validity map)

    # ---- which solver back end ------------------------------------------------------------------
    def _fused_specs(self):
        """Parameters of the device back end -- dict(reweight, huber_k, n_irls, thr, min_frac, n_draw, sobol_u) -- when the
        config's estimator / subsampler / re-detection callables are the weighted LSq / IRLS estimators, the Sobol-n draw and
        the inlier-fraction test: tagged by woft_amd.presets, or found to BEHAVE as those (woft_amd.probe: reference-format
        configs define them inline, configs/..._wLSq.py:14-53); else None (callable back end: the config's own functions run)."""
        self.solver_decision = None
        spec = self._fused_specs_plain()
        if self.visibility_mode is not None:
            self.solver_decision += (f"; visibility {self.visibility_mode}"
                                     + (f" (p > {self.visibility_thr:.9g})" if self.visibility_mode == "gate" else " (w * p)"))
        if self.fb_check:
            self.solver_decision += (f"; forward-backward check {self.fb_check} (|f + b|^2 <= {self.fb_alpha:.9g} * (|f|^2 + |b|^2) "
                                     f"+ {self.fb_beta:.9g})")
        if self._photo is not None:
            self.solver_decision += self._photo_decision("re-detected")
        return spec

    def _fused_specs_plain(self):
        C = self.C
        self.solver_decision = "callable back end"
        if os.environ.get("WOFT_FUSED", "1") == "0" or not config_get(C, "device_solver", True):
            self.solver_decision += " (device back end switched off)"
            return None
        if C.post_hoc_weights_postprocessing_fn or C.flow_numpy_out:
            return None
        if not hasattr(self.flower, "pin_source"):
            return None
        if not self._device_solver_reads(self.flower.C.raft_type):
            return None
        from .probe import solver_spec
        spec, how = solver_spec(C.H_estimator, C.subsampler_fn or None, C.redet_success_fn, device=self.device)
        self.solver_decision = ("device back end" if spec is not None else "callable back end") + f" ({how})"
        # A decision taken by PROBING replaces the config's own callables with the device solver on the strength of what they did
        # on synthetic inputs (woft_amd.probe): said at WARNING level, with the way out.  Tagged presets / no replacement: INFO.
        probed = spec is not None and "probed" in how
        logger.log(logging.WARNING if probed else logging.INFO,
                   f"tracker solver: {self.solver_decision}"
                   + (" -- the config's estimator / subsampler / re-detection callables were recognised by behavioural probing and "
                      "are replaced by the HIP solver (same results, tested); set `device_solver = False` in the tracker config "
                      "(or WOFT_FUSED=0) to run the config's own callables instead" if probed else ""))
        if spec is None:
            return None
        from .presets import sobol_points
        n_draw = spec["n_draw"]
        spec["sobol_u"] = torch.from_numpy(sobol_points(n_draw).astype(np.float32)).to(self.device) if n_draw else None
        return spec

    def _device_solver_reads(self, raft_type):
        """Whether the device back end can take its weights (and its visibility) from a provider of this raft_type."""
        return raft_type == ("weighted" if self.visibility_mode is None else "weighted_masked")

    # ---- public surface (TRK:19-57) -----------------------------------------------------------------
    def init(self, img, mask, img_identifier=None):
        k = self.C.downscale_inputs
        if k:                                                        # TRK:27-30
            img = ops.resize_by_factor_u8(_device_u8(img), k)
            mask = ops.resize_by_factor_u8(_device_u8(mask), k)
            img_identifier = None
        mask_np = mask.cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
        inside = mask_np > 0
        assert _count_components(inside) == 1                        # TRK:36-37 (single contour)
        self.template_img = img
        self.np_template_mask = mask_np
        self._local_chain = None
        self._warm = None
        self.template_mask = torch.from_numpy(inside).to(self.device)
        self._template_mask_u8 = torch.from_numpy(inside.astype(np.uint8) * 255).to(self.device)
        if hasattr(self.flower, "pin_source"):
            self.flower.pin_source(self.template_img)
            # Only correspondences that start inside the template mask survive the keep rule (TRK:287-312): the flow
            # weights of the other template pixels are never read by this tracker, and the weight head has no
            # cross-pixel terms (weighted_raft.py:363-383), so for flows FROM the template it is evaluated on the mask's
            # pixels only -- bit-identical weights there, identical homographies (tested), ~25 % fewer milliseconds per
            # frame at a quarter-frame mask.  Only the tracker's own calls ask for the region (`weight_region=True`, _flow
            # below): `compute_flow` called directly returns the full weight map; config key mask_weight_head = False
            # evaluates the head everywhere for the tracker too, as the reference's network does.
            if hasattr(self.flower, "pin_weight_region"):
                self.flower.pin_weight_region(inside if self._mask_weight_head() else None)
            # The same keep rule bounds the FLOW this tracker reads of a template flow: the update block is a stack of small
            # convolutions, so the last refinement iterations run only on the part of the 1/8-resolution map the mask's bounding
            # rectangle depends on (flow_provider.pin_flow_region; 11 cells more per iteration going backwards) -- identical
            # flow, correspondences and weights inside the mask, identical homographies (tested).  Asked for by the global
            # stage's own calls only (_global_stage), with the weight head's switch: mask_weight_head = False keeps the
            # reference's whole work.  Not with a visibility mode (the mask head reads every pixel) nor with the warm start.
            if hasattr(self.flower, "pin_flow_region"):
                self.flower.pin_flow_region(inside if self._flow_region_on() else None)
            # ... and with a subsampler in front of the fit (the default config draws 500 correspondences), only the weights
            # of the DRAWN correspondences are read, and the draw does not depend on the weights: the head is evaluated after
            # the selection, on the windows under the drawn pixels' upsampling support (config key sparse_weight_head =
            # False / env WOFT_SPARSE_WH=0: on the whole mask region, as above).  Identical homographies (tested).
            on = bool(config_get(self.C, "sparse_weight_head", os.environ.get("WOFT_SPARSE_WH", "1") != "0"))
            # (a visibility mode: the mask head runs on every pixel after the weight head and the provider defers nothing for a
            #  'weighted_masked' network -- the non-deferred path)
            self._sparse_weights = bool(on and self._fused is not None and self._fused["n_draw"] and self._mask_weight_head()
                                        and hasattr(self.flower, "finish_weights") and self.visibility_mode is None
                                        and not self.fb_check)
        if self._photo is not None:
            from .photo import PhotoTemplate
            self._photo_template = PhotoTemplate(self._photo_image(self.template_img), inside, stride=self._photo["stride"])
        self._set_pose(_EYE.copy(), good=True)
        self.prev_img, self.prev_img_identifier = img, img_identifier
        self.lost, self.N_lost = False, 0
        self._replay = None

    def set_fast_meta(self, meta):
        """Next track() call replays a stored result instead of computing flow (TRK:49-55)."""
        if self.C.downscale_inputs:
            raise NotImplementedError("Fastforward not compatible with input downscaling yet.")
        self._replay = meta

    @property
    def fast_forward(self):
        return self._replay is not None

    @fast_forward.setter
    def fast_forward(self, value):
        """Reference-style `tracker.fast_forward = False` (TRK:47,55,64) cancels a pending replay; True without a stored
        meta has nothing to replay (set_fast_meta is the way in)."""
        if not value:
            self._replay = None
        elif self._replay is None:
            raise ValueError("fast_forward = True needs set_fast_meta(meta)")

    def track(self, input_img, debug=False, img_identifier=None):
        if self.C.downscale_inputs:                                  # TRK:60-61
            input_img = ops.resize_by_factor_u8(_device_u8(input_img), self.C.downscale_inputs)
        if self._replay is not None:                                 # TRK:63-76
            meta, self._replay = self._replay, None
            self._warm = None
            H_cur2init = meta.estim_H_current2template
            self.lost, self.N_lost = False, 0
            self.prev_H2init = self.last_good_H2init = H_cur2init
            self.prev_img = input_img.clone() if isinstance(input_img, torch.Tensor) else np.array(input_img)
            self.prev_img_identifier = img_identifier
            return H_cur2init, meta

        meta = SimpleNamespace()
        self._n_tracked += 1
        if self.C.no_prewarp_after_N and self.N_lost > self.C.no_prewarp_after_N:
            self.last_good_H2init = _EYE.copy()                      # TRK:78-79
        meta.last_good_H2init = self.last_good_H2init.copy()
        # (becomes prev_img: the reference keeps a copy.  Host frames go through the pinned double buffer)
        frame = _device_u8(input_img, copy=True) if isinstance(input_img, torch.Tensor) else self._upload(input_img)

        prewarp_H = self.last_good_H2init
        fit = self._global_stage(frame, prewarp_H)
        if self._vis_mode is not None:
            meta.n_kept = self.n_kept                                # kept by the masks and the gate, template -> frame flow
        H_global = compose_H(prewarp_H, fit.H)
        meta.H_global_cur2init = H_global.copy()
        logger.debug(f"global_H_success: {fit.success}")
        H_cur2init = H_global
        if fit.success:
            self.lost, self.N_lost = False, 0
            self._warm = None                                        # (a re-detected frame ends the run: nothing to carry)
        else:
            self.lost, self.N_lost = True, self.N_lost + 1
            if not self.C.no_local_H:
                H_cur2init = meta.H_local_cur2init = self._local_stage(frame)
                meta.local_warm_started = self.local_warm_started    # (False without `warm_start_local`)
                if self._vis_mode is not None:
                    meta.n_kept_local = self.n_kept                  # ... frame t-1 -> t flow (None: no flow ran)
        if self._photo is not None and not self.lost:
            meta.H_flow_cur2init = H_cur2init.copy()                 # (the correspondence fit's pose, un-refined)
            H_cur2init = self._photo_stage(frame, H_cur2init, meta)
        if debug:
            logger.debug("debug visualisation (TRK:210-264) needs the OpenCV GUI and is not part of the HIP path")

        self.prev_img, self.prev_img_identifier = frame, img_identifier
        self._set_pose(H_cur2init.copy(), good=not self.lost)
        meta.lost, meta.N_lost, meta.global_H_success = self.lost, self.N_lost, fit.success
        self._announce(meta, self)
        k = self.C.downscale_inputs
        if k:                                                        # TRK:280-283
            H_cur2init = compose_H(np.diag([1.0 / k, 1.0 / k, 1.0]), H_cur2init, np.diag([float(k), float(k), 1.0]))
        return H_cur2init, meta

    def _mask_weight_head(self):
        if self.C.post_hoc_weights_postprocessing_fn:     # (a spatial filter of the weight MAP would read outside the mask)
            return False
        return bool(config_get(self.C, "mask_weight_head", os.environ.get("WOFT_MASK_WEIGHT_HEAD", "1") != "0"))   # (absent: on)

    def _flow_region_on(self):
        return bool(self._mask_weight_head() and self.visibility_mode is None and not self.warm_start_local and not self.fb_check)

    def _decision_for_meta(self):
        return self.solver_decision

    def _announce(self, meta, state):
        """On the first tracked frame of `state` (the tracker, or one target): which arithmetic and solver produced the results."""
        if state._announced:
            return
        state._announced = True
        meta.precision = getattr(self.flower, "precision", None)
        meta.precision_source = getattr(self.flower, "precision_source", None)
        meta.solver_decision = self._decision_for_meta()
        if self.visibility_mode is not None:          # (like n_kept: the field exists only with a mode)
            meta.visibility_mode = self.visibility_mode
        if self.fb_check:
            meta.fb_check = self.fb_check

    def _set_pose(self, H, good, state=None):
        state = state or self
        state.prev_H2init = H
        if good:
            state.last_good_H2init = H.copy()

    # ---- the two flow stages ------------------------------------------------------------------------
    def _flow(self, src, dst, src_is_previous_dst=False, flow_init=None, iters=None, flow_region=False):
        """-> (grid coords (2, n) int64, target coords (2, n) f32, weights (1, n) f32 | None, visibility probabilities (1, n) f32 |
        None (a visibility mode only), (gh, gw)); borrowed buffers of the provider: consumed before the next flow."""
        # (borrowed buffers, and -- only for THIS caller -- weights restricted to the region pinned in init(): a direct
        #  compute_flow() call by anybody else returns the full weight map, as the reference's does)
        kw = {"borrow": True, "weight_region": True} if hasattr(self.flower, "pin_source") else {}
        if self._sparse_weights:
            # both stages: the template flow on its mask region, the frame t-1 -> t flow of a lost frame on the pixels of
            # the carried mask (TRK:314-327) -- either way only the drawn correspondences' weights are read (_solve_device)
            kw["defer_weights"] = int(self._fused["n_draw"])
        if src_is_previous_dst and "borrow" in kw:
            kw["src_is_previous_dst"] = True
        if flow_region and hasattr(self.flower, "pin_flow_region"):
            kw["flow_region"] = True                                 # (flows from the pinned template only: the global stage)
        if flow_init is not None:                                    # (warm start: the local stage only)
            kw["flow_init"] = flow_init
            if iters is not None:
                kw["iters"] = iters
        self.n_kept = None
        p = None
        if self.visibility_mode is not None:
            # the tracker's own request: the fourth value is the visibility probability (the sigmoid of the mask logits, taken in the
            # mask's upsampling call) -- compute_flow called by anybody else returns the logits, as the reference's does
            src_xy, dst_xy, w, p = self.flower.compute_flow(src, dst, mode="TC", vis=False, src_img_identifier=None,
                                                            do_sigmoid=True, visibility=True, **kw)
        elif self.fb_check:
            src_xy, dst_xy, w, p = self._flow_fb(src, dst, kw)
        else:
            src_xy, dst_xy, w = self.flower.compute_flow(src, dst, mode="TC", vis=False, src_img_identifier=None,
                                                         do_sigmoid=True, **kw)
        s = getattr(self.flower, "last_flow_shape", None)
        return src_xy, dst_xy, w, p, ((s["H"], s["W"]) if s else None)

    def _flow_fb(self, src, dst, kw):
        """The flow src -> dst as _flow asks for it, the reverse flow dst -> src, and their forward-backward verdict on the flow
        grid: -> (src_xy, dst_xy, w, ok (1, n) 0/1 floats).  The forward call is the one a tracker without fb_check makes (same
        correspondences and weights, bit for bit) plus the flow map of the same upsampling launch; its results are copied before
        the reverse flow overwrites the provider's per-size output buffers.  The reverse flow reads no weights."""
        f = self.flower
        src_xy, dst_xy, w = f.compute_flow(src, dst, mode="TC", vis=False, src_img_identifier=None, do_sigmoid=True,
                                           keep_flow=True, **kw)
        fwd, dst_xy, w = f.flow_map().clone(), dst_xy.clone(), (None if w is None else w.clone())
        # (the warm start carries the FORWARD flow: read before the reverse flow replaces the provider's last-flow state)
        self._fb_low = (f.flow_low(), f.last_flow_key) if self.warm_start_local else None
        bwd = f.compute_flow(dst, src, mode="flow", vis=False, src_img_identifier=None, borrow=True, skip_weights=True)[0]
        _, ok = ops.flow_fb(fwd, bwd, self.fb_alpha, self.fb_beta, want_err=False)
        return src_xy, dst_xy, w, ok.reshape(1, -1)

    def _global_stage(self, frame, prewarp_H):
        """Template -> frame pre-warped by the last good homography (TRK:85-162).  Kept: correspondences that start
        in the template mask, land inside the frame and (unless do_not_mask_TCs_by_prewarped) on a pixel the pre-warp
        actually filled."""
        valid = None
        if np.array_equal(prewarp_H, _EYE):
            prewarped = frame                                        # identity warp: same image, every pixel filled
        else:
            # (two per-size buffers, reused: consumed by the flow / the selection before the next frame's warp is enqueued on
            #  the same stream; allocating them per frame was ~15 us of host time in front of the frame's first kernel)
            prewarped, valid = self._prewarp.lookup(tuple(frame.shape), lambda: (
                torch.empty_like(frame), torch.empty(frame.shape[:2], dtype=torch.uint8, device=self.device)))
            ops.warp_perspective_u8(frame, prewarp_H, prewarped, valid)
        if self.C.do_not_mask_TCs_by_prewarped:
            valid = None
        src_xy, dst_xy, w, p, grid = self._flow(self.template_img, prewarped, flow_region=self._flow_region_on())
        return self._solve(src_xy, dst_xy, w, grid, frame.shape[:2], self._template_mask_u8, valid, bounds=True,
                           judge=True, vis=p)

    def _local_stage(self, frame):
        """Frame t-1 -> frame t, chained onto the previous pose (TRK:171-207).  Kept: correspondences that start in
        the template mask carried to frame t-1 (nearest-neighbour warp by inv(prev_H2init), TRK:314-327).  A failed
        fit keeps the previous pose."""
        # consecutive lost frames: frame t-1 was the TARGET of the previous local flow and is the SOURCE of this one -- the provider
        # then takes its feature map from that flow instead of encoding the same image again (identical values)
        chained = (self._local_chain is not None and self._local_chain[0] is self.prev_img and self._local_chain[1] == self._n_tracked - 1
                   and os.environ.get("WOFT_LOCAL_REUSE", "1") != "0")
        init, self.local_warm_started = None, False
        if self.warm_start_local:
            # warm start: the previous track() ran this stage too, its flow belonged to frames (t-2, t-1) -- `chained`, whatever
            # WOFT_LOCAL_REUSE says -- and ran in the buffer set and padding geometry this one will (equal flow keys)
            ran = (self._local_chain is not None and self._local_chain[0] is self.prev_img
                   and self._local_chain[1] == self._n_tracked - 1)
            if ran and self._warm is not None and self._warm[1] == self.flower.flow_key(self.prev_img):
                from .warm import forward_interpolate
                init = forward_interpolate(self._warm[0])
            self.local_warm_started = init is not None
        src_xy, dst_xy, w, p, grid = self._flow(self.prev_img, frame, src_is_previous_dst=chained, flow_init=init,
                                                iters=self.warm_start_iters)
        self._local_chain = (frame, self._n_tracked)
        if self.warm_start_local:
            self._warm = self._fb_low if self.fb_check else (self.flower.flow_low(), self.flower.last_flow_key)
        if np.array_equal(self.prev_H2init, _EYE):
            prev_mask = self._template_mask_u8
        else:
            prev_mask = torch.empty_like(self._template_mask_u8)
            ops.warp_perspective_u8(self._template_mask_u8, np.linalg.inv(self.prev_H2init), prev_mask, None,
                                    nearest=True)
        return self._local_fit(src_xy, dst_xy, w, grid, frame.shape[:2], prev_mask, p)

    def _local_fit(self, src_xy, dst_xy, w, grid, hw, prev_mask, vis, undo=None):
        """The tail of the local stage: the fit (no re-detection test), chained onto the previous pose; `undo` takes a window's
        H back to frame coordinates.  A failed fit (the estimator only: anything else is an error) keeps the previous pose."""
        try:
            fit = self._solve(src_xy, dst_xy, w, grid, hw, prev_mask, None, bounds=False, judge=False, vis=vis)
            if not np.all(np.isfinite(fit.H)):
                raise FloatingPointError("singular homography system")
            return compose_H(fit.H if undo is None else undo(fit.H), self.prev_H2init)
        except Exception as ex:
            logger.warning(f"frame-to-frame homography failed ({type(ex).__name__}): pose of the previous frame kept")
            return self.prev_H2init

    # ---- the solver ---------------------------------------------------------------------------------
    def _solve(self, src_xy, dst_xy, w, grid, frame_hw, src_mask_u8, dst_valid_u8, bounds, judge, vis=None):
        """Prune the dense field and fit H (target -> source coordinates); judge: also run the re-detection test.
        vis (a visibility mode): the probabilities on the flow grid, applied inside the keep rule / the weights by either back end."""
        Hh, Ww = frame_hw
        grid = grid or (Hh, Ww)
        try:
            if self._fused is not None:
                return self._solve_device(dst_xy, w, grid, (Hh, Ww), src_mask_u8, dst_valid_u8, bounds, vis)
            return self._solve_callables(src_xy, dst_xy, w, grid, (Hh, Ww), src_mask_u8, dst_valid_u8, bounds, judge, vis)
        except AssertionError:
            # Too few correspondences for a fit (least_squares_H.py:162).  Without a visibility mode this is the reference's
            # behaviour: the global stage lets it out of track(), the local stage keeps the previous pose.  A gate is MEANT to empty
            # the set under occlusion: the global stage then reports a failed re-detection (H = identity: the pre-warp's pose) and
            # the frame is lost, as any other frame whose global fit is rejected.
            if self._vis_mode is None or not judge or self.n_kept is None or self.n_kept >= 4:
                raise
            logger.debug(f"global stage: {self.n_kept} correspondences after the "
                         + (f"forward-backward {self.fb_check}" if self.fb_check else f"visibility {self.visibility_mode}") + ": no fit")
            return _Fit(H=_EYE.copy(), success=False)

    def _solve_device(self, dst_xy, w, grid, frame_hw, src_mask_u8, dst_valid_u8, bounds, vis=None):
        F, n_grid = self._fused, grid[0] * grid[1]
        cap = 1024 if F["n_draw"] else n_grid                        # (a Sobol draw selects at most 1024)
        blk = (b := self._buffers.lookup((1, n_grid, cap), lambda: PlanarBuffers(F, 1, n_grid, cap, self.device, False))).block
        weighted = F.get("weighted", True)
        if vis is not None:
            # (an unweighted estimator under 'weight': the output weight is p itself and the fit is called weighted)
            ops.tc_select_vis(dst_xy, w if weighted else None, src_mask_u8, dst_valid_u8, frame_hw[0], frame_hw[1], bounds,
                              F["sobol_u"], vis, self._vis_mode, self._vis_thr, b.ws, b.pa, b.pb, b.w, blk.count, grid=grid)
            weighted = weighted or self._vis_mode == "weight"
        else:
            ops.tc_select(dst_xy, w, src_mask_u8, dst_valid_u8, frame_hw[0], frame_hw[1], bounds, F["sobol_u"], b.ws,
                          b.pa, b.pb, b.w, blk.count, grid=grid)
            # Deferred weights (w is None): the correspondences the fit will read are decided by the flow alone (masks, bounds,
            # Sobol draw), so they were selected first; now the provider evaluates the weight head on the windows under THEIR
            # upsampling support only and hands back the weights of exactly these pixels (exact: the head has no cross-pixel
            # terms) -- identical fit.  An UNWEIGHTED estimator (the reference's "plainLSq" configs call the library with
            # weights=None) reads no weight at all: the deferred head is then simply never evaluated.
            if w is None and weighted and getattr(self.flower, "weights_deferred", False):
                self.flower.finish_weights(b.pb, blk.selected, b.cap, out=b.w)                     # (pb: the source pixels)
        fit_and_judge(F, b, weighted)
        self.host_wait_s += blk.read()                    # (bench: wall time minus this = the launch loop's host time per frame)
        (fit, selected, self.n_kept, _), = decode(blk.host.numpy(), 1, F, False)
        if fit is None:
            raise AssertionError(torch.Size([1, selected, 2]))       # least_squares_H.py:162 (fewer than 4 points; TRS: than 2)
        return fit

    def _solve_callables(self, src_xy, dst_xy, w, grid, frame_hw, src_mask_u8, dst_valid_u8, bounds, judge, vis=None):
        C = self.C
        post = None
        if C.post_hoc_weights_postprocessing_fn:
            post = self.flower.postprocess_weights(w.clone(), C.post_hoc_weights_postprocessing_fn)
        if vis is None:
            keep = ops.tc_flags(dst_xy if bounds else None, src_mask_u8, dst_valid_u8, frame_hw[0], frame_hw[1], bounds,
                                grid=grid)
        else:
            keep = ops.tc_flags_vis(dst_xy if bounds else None, src_mask_u8, dst_valid_u8, frame_hw[0], frame_hw[1], bounds,
                                    vis, self._vis_mode, self._vis_thr, grid=grid)
        pick = lambda t: None if t is None else t[:, keep]
        src_xy, dst_xy, w, post = pick(src_xy), pick(dst_xy), pick(w), pick(post)
        if vis is not None:
            self.n_kept = int(src_xy.shape[1])
            if self.n_kept == 0:                                     # (nothing to hand to the config's callables)
                raise AssertionError(torch.Size([1, 0, 2]))
            if self._vis_mode == "weight":                           # w * p in fp32 on the compacted set; p alone without weights
                pk = vis.reshape(1, -1)[:, keep]
                w = pk if w is None else w * pk
        if judge:
            src_xy = src_xy.float()                                  # TRK:131 (global stage); the local stage hands the
                                                                     # subsampler the int64 grid coordinates (TRK:186-193)
        if C.flow_numpy_out and not judge:                           # (the reference asks numpy of the local flow only)
            to_np = lambda t: None if t is None else t.cpu().numpy()
            src_xy, dst_xy, w, post = to_np(src_xy), to_np(dst_xy), to_np(w), to_np(post)
        if C.subsampler_fn:
            src_xy, dst_xy, w, post = C.subsampler_fn(src_xy, dst_xy, w, post)
        if not judge:
            src_xy = src_xy.float() if isinstance(src_xy, torch.Tensor) else src_xy.astype(np.float32)
        H = C.H_estimator(dst_xy.T[None], src_xy.T[None], w)
        H = H.float() if isinstance(H, torch.Tensor) else torch.as_tensor(np.asarray(H)).float()
        fit = _Fit(H=H.detach().cpu().numpy()[0].astype(np.float64), success=None)
        if judge:
            fit.success = bool(C.redet_success_fn(H, src_xy, dst_xy, post if post is not None else w))
        return fit


class WOFTWindow(YAOFTrackerSingleControl):
    """The reference's search-window tracker (pytracking/tracker/WOFT_window.py, WIN below): YAOFTrackerSingleControl with one
    more config key, `search_window_margin`.  The template -> frame flow runs on the template mask's box plus that margin, fixed
    at init() (WIN:37-44); the frame t-1 -> t flow of a lost frame on the box of the mask carried to frame t-1, plus the same
    margin (WIN:212-221); a homography fitted between two crops goes back to frame coordinates through H_undo_crop (WIN:420-427).
    State machine, solver back ends, weight-head shortcuts and the host-frame path are the parent's; only the two stages differ.

    What differs from WIN, on purpose ("Search window"): a box that the minimum-size step pushes past the frame edge
    is cut to the frame (WIN slices with a negative index there).  `search_bbox` / `local_search_bbox` hold the boxes in use
    (woft_amd.window.Box; the local one is None on a frame that was not lost)."""
    PLAN_BOUND = 4                    # local-window shapes the flow provider keeps besides the pinned global window
    MIN_FLOW_SIDE = 16                # a local window cut smaller than this by the frame edge: no flow, previous pose kept

    BUFFER_SETS = PLAN_BOUND + 1      # (the parent keeps ONE grid size; here the global and the local windows alternate)
    REFUSED_BY = "search-window tracker"
    REFUSED = (
        # (not built: the window stages have their own _flow call sites and per-window plans)
        ("fb_check", "only YAOFTrackerSingleControl runs the reverse flow"),
        # (the local windows move with the object: the flow of one window is not on the grid of the next)
        ("warm_start_local", "its frame t-1 -> t flows run on a window that follows the object, so consecutive flows do not share "
                             "a grid"),
    )

    def __init__(self, config):
        super().__init__(config)
        self.search_bbox = self.local_search_bbox = None
        if hasattr(self.flower, "bound_plans"):
            self.flower.bound_plans(self.PLAN_BOUND)

    def init(self, img, mask, img_identifier=None):
        from . import window
        super().init(img, mask, img_identifier)                      # (downscaling, single-contour check, state: the parent's)
        inside = self.np_template_mask > 0
        Hh, Ww = inside.shape
        self._margin = self.C.search_window_margin or None           # (absent key: an empty, falsy Config)
        self._template_box = window.Box.from_mask(inside)
        self.search_bbox = window.search_box(self._template_box, self._margin, Ww, Hh)
        self.local_search_bbox = None
        self._rect = rect = self.search_bbox.crop_rect()
        y0, x0, rows, cols = rect
        self._template_crop = ops.crop_u8(_device_u8(self.template_img), rect)
        self._template_mask_crop = ops.crop_u8(self._template_mask_u8, rect)
        if hasattr(self.flower, "pin_source"):                       # the parent pinned the whole template: re-pin the crop
            self.flower.pin_source(self._template_crop)
            if hasattr(self.flower, "pin_weight_region"):
                self.flower.pin_weight_region(inside[y0:y0 + rows, x0:x0 + cols] if self._mask_weight_head() else None)

    def track(self, input_img, debug=False, img_identifier=None):
        self.local_search_bbox = None
        return super().track(input_img, debug=debug, img_identifier=img_identifier)

    def _global_stage(self, frame, prewarp_H):
        """Template crop -> the search window of the frame pre-warped by the last good homography (WIN:101-193): the window's
        pixels of the pre-warp and of its validity map are all that is computed.  The keep rule runs in window coordinates with
        the window's size as bounds (WIN:335-366), the re-detection test on the window-coordinate homography (WIN:191)."""
        from . import window
        rect = self._rect
        rows, cols = rect[2], rect[3]
        prewarped, valid = self._prewarp.lookup((rows, cols), lambda: (
            torch.empty((rows, cols, frame.shape[2]), dtype=torch.uint8, device=self.device),
            torch.empty((rows, cols), dtype=torch.uint8, device=self.device)))
        if np.array_equal(prewarp_H, _EYE):
            ops.crop_u8(frame, rect, prewarped)                      # identity warp: the frame's own pixels, all of them filled
            valid = None
        else:
            ops.warp_perspective_window_u8(frame, prewarp_H, rect, prewarped, valid)
        if self.C.do_not_mask_TCs_by_prewarped:
            valid = None
        src_xy, dst_xy, w, p, grid = self._flow(self._template_crop, prewarped)
        fit = self._solve(src_xy, dst_xy, w, grid, (rows, cols), self._template_mask_crop, valid, bounds=True, judge=True, vis=p)
        fit.H = window.H_undo_crop(self.search_bbox, fit.H)
        return fit

    def _carried_mask_box(self):
        """-> (template mask carried to frame t-1 (device uint8), its Box): nearest-neighbour warp by inv(prev_H2init) and the
        bounding box of the result in one launch, one five-integer device -> host read (lost frames only)."""
        from . import window
        if np.array_equal(self.prev_H2init, _EYE):
            return self._template_mask_u8, self._template_box
        prev_mask = torch.empty_like(self._template_mask_u8)
        if not self._margin:                                         # whole-frame window: nobody needs the box
            ops.warp_perspective_u8(self._template_mask_u8, np.linalg.inv(self.prev_H2init), prev_mask, None, nearest=True)
            return prev_mask, None
        bbox = ops.mask_bbox(self._template_mask_u8, Hmat=np.linalg.inv(self.prev_H2init), warped=prev_mask)
        rmin, rmax, cmin, cmax, any_set = bbox.cpu().tolist()
        return prev_mask, window.Box.from_extent(rmin, rmax, cmin, cmax, bool(any_set))

    def _local_stage(self, frame):
        """Frame t-1 -> frame t on the box of the carried template mask plus the margin (WIN:208-255), chained onto the previous
        pose.  A failed fit -- or a window the frame edge leaves no room for -- keeps the previous pose."""
        from . import window
        Hh, Ww = frame.shape[:2]
        prev_mask, mask_box = self._carried_mask_box()
        box = self.local_search_bbox = window.search_box(mask_box, self._margin, Ww, Hh)
        rect = box.crop_rect()
        if min(rect[2], rect[3]) < self.MIN_FLOW_SIDE:
            logger.warning(f"local search window {box} leaves a {rect[2]} x {rect[3]} crop: no flow, pose of the previous frame kept")
            return self.prev_H2init
        prev_win = ops.crop_u8(_device_u8(self.prev_img), rect)
        cur_win = ops.crop_u8(frame, rect)
        mask_win = ops.crop_u8(prev_mask, rect)
        src_xy, dst_xy, w, p, grid = self._flow(prev_win, cur_win)
        return self._local_fit(src_xy, dst_xy, w, grid, (rect[2], rect[3]), mask_win, p, undo=lambda H: window.H_undo_crop(box, H))
