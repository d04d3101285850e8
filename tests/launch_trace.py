"""Launch traces: every call into libwoft_hip.so in canonical form (helper of test_launch_trace_gpu.py, not collected).

A `LibProxy` stands in for the loaded library (woft_amd._lib._lib) for the duration of a block, records every call and forwards
it unchanged.  Canonical form of a call: scalars by value (floats as float.hex()), pointers as small integers -- 0 for NULL, else
numbered by first appearance within the trace -- for void* arguments, void* fields and void*[4] arrays of the parameter structs
(reached through the byref object's _obj), pointer tables and the stream.  Argument and field types come from _lib._SIGS and the
structs' _fields_.  A trace therefore pins which launches run, in which order, with which arguments, and which buffers alias which,
independent of addresses and of allocation order.

tests/golden/launch_traces.json holds, per scenario and per call, "<entry point> <crc32 of the canonical form> <summary>", and the
CRC32 of the scenario's outputs where two runs of the recording commit agreed on it.  The fixture is a record of what the engine
launched at the commit BEFORE a change of the host code (`python tests/launch_trace.py --record` there): a refactor of the host
code passes against it unchanged; a change that moves launches on purpose re-records it and shows the moved launches in its diff.

The tracker scenarios (tracker_*, window_lost, chained*) run a whole tracker for three frames.  Their fixture entries hold only the
lines of the entry points outside the engine (PLANAR below) and of everything FlowProvider.finish_weights calls; pointers are
still numbered over the WHOLE trace, engine calls included, so a kept line's aliasing with the engine's buffers is pinned too.
Between those lines stands one "d2h" line per device-to-host copy of the track() calls (d2h_copies), in program order: the number
of reads per frame is part of the trace.
"""
import ctypes as C
import json
import sys
import zlib
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from woft_amd import _lib, synth  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "launch_traces.json"
_FLOATS = (C.c_float, C.c_double)


class LibProxy:
    """Records (name, canonical arguments, summary) of every call of a declared entry point, then forwards it."""

    def __init__(self, lib):
        self._real, self.calls, self._ids = lib, [], {}
        self.only, self.inside = None, 0         # tracker scenarios: keep calls of these name prefixes, or made while `inside`

    def _pointer(self, v):
        v = v.value if isinstance(v, C.c_void_p) else v
        return 0 if not v else self._ids.setdefault(int(v), len(self._ids) + 1)

    def _value(self, ctype, v):
        if isinstance(v, C.Array):                               # pointer tables, index / size arrays, double[9]
            return [self._value(v._type_, x) for x in v]
        if ctype is C.c_void_p or v is None:
            return self._pointer(v)
        if ctype in _FLOATS:
            return ctype(v).value.hex()                          # (the value the callee sees: a float argument is rounded to fp32)
        if hasattr(ctype, "_type_") and hasattr(ctype._type_, "_fields_"):      # POINTER(struct), passed as byref(struct)
            return self._struct(v._obj)
        if hasattr(ctype, "_type_") and not isinstance(ctype._type_, str):      # POINTER(c_double) given an array: above
            return self._pointer(C.cast(v, C.c_void_p))
        return int(v)

    def _struct(self, s):
        return {name: self._value(ftype, getattr(s, name)) for name, ftype in s._fields_}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        sig = _lib._SIGS.get(name)
        if sig is None:
            return fn

        def call(*args):
            assert len(args) == len(sig[1]), name
            canon = [self._value(t, a) for t, a in zip(sig[1], args)]      # (always: pointers are numbered over the whole trace)
            # (a *_ws_bytes size query is no launch, and a scratch cached per process asks only once)
            if self.only is None or self.inside or (name.startswith(self.only) and not name.endswith("_ws_bytes")):
                self.calls.append((name, canon, _summary(args)))
            return fn(*args)
        self.__dict__[name] = call
        return call


def _summary(args):
    """Readable part of a fixture line: the fields a change of the launch programs is most likely to move."""
    out = []
    for a in args:
        s = getattr(a, "_obj", None)
        if isinstance(s, _lib.ConvParams):
            out.append(f"halo={s.halo} epi={s.epi} cout={s.cout} {s.ho}x{s.wo} roi={s.roi_y0},{s.roi_x0},{s.roi_h},{s.roi_w}")
        elif isinstance(s, _lib.LookupOtfParams):
            out.append(f"roi={s.roi_y0},{s.roi_x0},{s.roi_h},{s.roi_w} smp={s.smp_y0},{s.smp_x0},{s.smp_h},{s.smp_w} "
                       f"fh_part={int(bool(s.fh_part))} need={int(bool(s.need))}")
        elif isinstance(s, _lib.LookupParams):
            out.append(f"levels={s.levels} radius={s.radius}")
    return " | ".join(out)


def lines(calls):
    """The fixture's form of a trace: one string per call."""
    return [f"{name} {zlib.crc32(json.dumps(canon, sort_keys=True).encode()):08x} {summary}".rstrip()
            for name, canon, summary in calls]


def first_difference(want, got):
    """-> None, or (index of the first differing call, the fixture's line, this run's line)."""
    for k in range(max(len(want), len(got))):
        a, b = (want[k] if k < len(want) else "<no call>"), (got[k] if k < len(got) else "<no call>")
        if a != b:
            return k, a, b
    return None


# ---- scenarios ------------------------------------------------------------------------------------------------------
def _config(sd, iters, precision, raft_type="weighted", small=False, corr=None, wh=None, mh=None):
    """The provider of tests/test_flow_gpu.py::_flow_config, padding_mode "nopad"."""
    from woft_amd.config import Config
    from woft_amd.flow_provider import RAFTWrapper
    c = Config()
    c.of_class = RAFTWrapper
    c.raft_type = raft_type
    c.class_params = Config()
    c.class_params.small = small
    c.class_params.mixed_precision = False
    c.class_params.alternate_corr = False
    c.class_params.weight_head_structure = wh or [(128, 3)] * 3
    if mh:
        c.class_params.mask_estimation = True
        c.class_params.mask_head_structure = mh
    c.model = sd
    c.iters = iters
    c.padding_mode = "nopad"
    c.precision = precision
    if corr:
        c.corr = corr
    return c.of_class(c)


def _pair(h, w, seq_id, n=2):
    """Template + frames as device tensors that live as long as the scenario: an upload freed inside the trace would hand its
    address to a later allocation, and the pointer numbering would depend on the allocator."""
    a = synth.make_template(h, w, seq_id=seq_id)
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in [a] + [synth.make_frame(a, t) for t in range(1, n)]]


def _one_flow(patch, **kw):
    prov = _config(synth.make_state_dict(seed=3, **kw.pop("sd", {})), kw.pop("iters"), kw.pop("precision"), **kw)
    a, b = _pair(128, 160, 2)
    return list(prov.compute_flow(a, b, mode="flow"))


def full_bf16x3_otf(patch):
    prov = _config(synth.make_state_dict(seed=3), 3, "bf16x3", corr="otf")
    a, b, c = _pair(128, 160, 2, 3)
    out = list(prov.compute_flow(a, b, mode="flow"))
    out += [t.clone() for t in prov.compute_flow(a, b, mode="flow", flow_init=torch.zeros(2, 16, 20))]
    out += [t.clone() for t in prov.compute_flow(b, c, mode="flow", src_is_previous_dst=True)]
    assert prov.source_features_reused
    return out


def switches_off(patch):
    from woft_amd import engine
    for name in ("PAIR_BRANCHES", "FOLD_GATHER", "DEFER_NORM", "PYRAMID_ONE_LAUNCH"):
        patch.setattr(engine, name, False)
    return _one_flow(patch, iters=3, precision="bf16x3")


def mask_head(patch):
    st = [(64, 3)]
    prov = _config(synth.make_state_dict(seed=3, mask_head_structure=st), 2, "bf16x3", raft_type="weighted_masked", mh=st)
    a, b = _pair(128, 160, 2)
    return list(prov.compute_flow(a, b, mode="flow", visibility=True))


def flow_region(patch):
    """The set-up of tests/test_flow_region_engine_gpu.py; outputs: the masked pixels only."""
    from pytracking.utils.config import load_config
    H, W = 256, 320
    mask = np.zeros((H, W), bool)
    mask[8:40, 264:296] = True
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT.py")
    conf.flow_config.model, conf.flow_config.iters, conf.flow_config.precision = synth.make_state_dict(seed=11), 4, "bf16x3"
    conf.flow_config.graph = False
    fl = conf.tracker_class(conf).flower
    template, frame = _pair(H, W, 4, 3)[::2]
    fl.pin_source(template)
    fl.pin_weight_region(mask)
    fl.pin_flow_region(mask)
    fl.defer_min_ratio = 0
    sel = torch.from_numpy(mask.reshape(-1)).cuda()
    ys, xs = np.nonzero(mask)
    pick = np.random.default_rng(0).choice(ys.size, 300, replace=False)
    pts = torch.from_numpy(np.stack([xs[pick], ys[pick]], 1).astype(np.float32)).cuda()
    count = torch.tensor([300], dtype=torch.int32, device="cuda")
    flow, w = fl.compute_flow(template, frame, mode="flow", do_sigmoid=True, weight_region=True, flow_region=True)
    assert fl.engine.plan(H, W).flow_region is not None
    out = [flow.reshape(2, -1)[:, sel], w.reshape(1, -1)[:, sel]]
    _, dst, none = fl.compute_flow(template, frame, mode="TC", do_sigmoid=True, weight_region=True, flow_region=True,
                                   defer_weights=300, borrow=True)
    assert fl.weights_deferred and none is None
    out.append(dst[:, sel])
    out.append(fl.finish_weights(pts, count, 300, out=torch.zeros(300, device="cuda")))
    return out


# ---- tracker scenarios: the planar stage of every tracker class and back end --------------------------------------------------
PLANAR = ("woft_tc_", "woft_hfit", "woft_inlier_frac", "woft_ransac", "woft_trs", "woft_chain_tc", "woft_flow_fb",
          "woft_warp_perspective", "woft_crop_u8", "woft_mask_bbox", "woft_wh_needed")


def d2h_copies(patch, on_copy):
    """For as long as `patch` (a pytest MonkeyPatch) holds: on_copy(name) after every device-to-host copy made through
    Tensor.cpu / .item / .tolist / .to / .copy_."""
    T = torch.Tensor
    real = {n: getattr(T, n) for n in ("cpu", "item", "tolist", "copy_", "to")}

    def d2h(name, is_copy):
        def wrapped(self, *a, **kw):
            out = real[name](self, *a, **kw)
            if is_copy(self, a, out):
                on_copy(name)
            return out
        return wrapped
    from_dev = lambda self, a, out: self.is_cuda
    patch.setattr(T, "cpu", d2h("cpu", from_dev))
    patch.setattr(T, "item", d2h("item", from_dev))
    patch.setattr(T, "tolist", d2h("tolist", from_dev))
    patch.setattr(T, "to", d2h("to", lambda self, a, out: self.is_cuda and not out.is_cuda))
    patch.setattr(T, "copy_", d2h("copy_", lambda self, a, out: not self.is_cuda and a[0].is_cuda))


def _never():
    from woft_amd import presets
    return presets.redetection_by_inliers(1e-6, 0.999)               # (a re-detection test no fit satisfies)


def _tracked(trk, frames, before=None):
    """track() over the frames with the planar filter and the read recorder on -> the scenario's outputs: every H as a float64
    tensor, lost / N_lost / n_kept (-1: None or no such field) as one int64 tensor per frame."""
    import pytest
    proxy = _lib._lib
    proxy.only = PLANAR
    fl = trk.flower
    if hasattr(fl, "finish_weights"):
        inner = fl.finish_weights

        def finish_weights(*a, **kw):
            proxy.inside += 1
            try:
                return inner(*a, **kw)
            finally:
                proxy.inside -= 1
        fl.finish_weights = finish_weights
    outs = []
    for k, f in enumerate(frames, 1):
        if before is not None:
            before(k)
        with pytest.MonkeyPatch.context() as p:
            d2h_copies(p, lambda name: proxy.calls.append(("d2h", [], name)))
            H, meta = trk.track(f)
        metas = meta if isinstance(meta, list) else [meta]
        ints = [[int(m.lost), int(m.N_lost), -1 if getattr(m, "n_kept", None) is None else int(m.n_kept)] for m in metas]
        ints.append([-1 if trk.n_kept is None else int(trk.n_kept)] * 3)
        outs += [torch.from_numpy(np.array(H, np.float64)), torch.tensor(ints, dtype=torch.int64)]
    return outs


_POOLS = []


def _private_pool(run):
    """Tracker scenarios free and allocate per frame (the cloned frame, the carried mask, a window's crops), and a pointer's
    number says which freed block a later allocation got.  In the process's shared caching allocator that depends on every
    tensor any earlier test left alive or cached; so the whole scenario allocates from a memory pool of its own, new and empty,
    where it depends on the scenario's own sequence of allocations alone."""
    def in_pool(patch):
        import gc
        from woft_amd import ops
        for name in ("_BBOX_WS", "_HFIT_WS", "_RANSAC_WS", "_TRS_WS"):     # (the process's scratch caches: the scenario makes
            patch.setattr(ops, name, {})                                   #  its own, in its pool, whatever ran before)
        gc.collect()
        torch.cuda.synchronize()
        pool = torch.cuda.MemPool()
        _POOLS.append(pool)                                          # (kept: a tensor that outlives the scenario keeps its memory)
        with torch.cuda.use_mem_pool(pool):
            try:
                return run(patch)
            finally:
                gc.collect()                                         # (the scenario's tensors go back to its pool, not to the next one's)
                torch.cuda.synchronize()
    return in_pool


def _tracker_scenario(cfg, edit=None, check=None, lost_from=None, mh=None):
    """A shipped tracker config on the synthetic checkpoint, 128 x 160, iters 1, no graph, three frames.  lost_from: the first
    frame from which the re-detection test always fails (the config is edited and _fused_specs() called again; the earlier spec
    is kept alive, so its Sobol table's address is not handed out again)."""
    def run(patch):
        from pytracking.utils.config import load_config
        conf = load_config(ROOT / "pytracking" / "configs" / cfg)
        fc = conf.flow_config
        fc.model = synth.make_state_dict(seed=7, **(dict(mask_head_structure=mh) if mh else {}))
        fc.iters, fc.graph = 1, False
        if edit is not None:
            edit(conf)
        trk = conf.tracker_class(conf)
        trk.flower.defer_min_ratio = 0                               # (the sparse weight head at this small size too)
        template, *frames = _pair(128, 160, 4, 4)
        trk.init(template, synth.make_init_mask(128, 160))
        if check is not None:
            check(trk)
        kept = []

        def before(k):
            if k == lost_from:
                kept.append(trk._fused)
                conf.redet_success_fn = _never()
                trk._fused = trk._fused_specs()
        return _tracked(trk, frames, before)
    return _private_pool(run)


def _set(**kw):
    def edit(conf):
        for k, v in kw.items():
            setattr(conf, k, v)
    return edit


def _is(**want):
    def check(trk):
        for k, v in want.items():
            got = getattr(trk, k)
            assert (got is not None) == v if k == "_fused" else got == v, (k, got, v)
    return check


def _visibility_gate(conf):
    conf.flow_config.raft_type = "weighted_masked"
    conf.visibility_mode = "gate"


def _chained_scenario(multi, **kw):
    """The chained trackers on the stub provider and the sizes of tests/chained_multi_util.py (48 x 64, deltas (None, 1, 2, 4));
    the stub's flows are kept alive for the scenario, as the frames are."""
    def run(patch):
        import chained_multi_util as U
        patch.setenv("WOFT_FUSED", "1")
        sub = kw.get("subsampler_fn", True)
        conf = U.stub_config(multi, estimator=kw.get("estimator"))
        if sub is None:
            conf.subsampler_fn = None
        trk = conf.tracker_class(conf)
        keep = _keep_flows(trk.flower)
        frame0, frames = U.stub_frames()
        masks = U.stub_masks()
        trk.init(frame0, masks if multi else masks[0])
        if multi:
            assert trk._route == kw["route"], trk._route
        outs = _tracked(trk, frames[:3])
        del keep[:]
        return outs
    return _private_pool(run)


def _ransac():
    from woft_amd import presets
    return presets.estimator_ransac(10000, 3.0, 0.995)


def _keep_flows(provider):
    """The stub provider's flows stay alive for the scenario, as the frames do -> the list that holds them."""
    keep, inner = [], provider.compute_flow

    def compute_flow(*a, **k):
        out = inner(*a, **k)
        keep.append(out)
        return out
    provider.compute_flow = compute_flow
    return keep


def _windowed(trk, frames):
    """Three frames of a windowed chained tracker whose R0 is a real window, not the frame."""
    assert trk.multi.rect0[2:] != tuple(frames[0].shape[:2]) and trk.multi.rect0[:2] != (0, 0), trk.multi.rect0
    keep = _keep_flows(trk.flower)
    outs = _tracked(trk, frames[:3])
    del keep[:]
    return outs


def _chained_window_scenario(patch):
    """WOFTChainedWindow, chain_prewarp on, on the stub provider, frames and mask of tests/test_chained_window_gpu.py (96 x 128,
    deltas (None, 1, 2, 4)): every chain unreliable, so the pre-warped direct candidate carries the pose."""
    import test_chained_window_gpu as W
    from pytracking.utils.config import load_config
    patch.setenv("WOFT_FUSED", "1")
    conf = load_config(ROOT / "pytracking" / "configs" / "WOFT_chained_window.py")
    conf.flow_config.of_class = lambda fc: W._MotionProvider(fc, "chained")
    conf.chain_deltas, conf.chain_window_min, conf.chain_window_quantum, conf.chain_prewarp = W.S_DELTAS, 32, 16, True
    assert conf.search_window_margin
    trk = conf.tracker_class(conf)
    trk.flower.tracker = trk
    trk.init(W._stub_frame(0), W._stub_mask())
    return _windowed(trk, [W._stub_frame(t) for t in range(1, 4)])


def _chained_multi_window_scenario(route, **kw):
    """WOFTChainedMultiWindow on the two-motion stub provider and the three masks of tests/test_chained_multi_window_gpu.py."""
    def run(patch):
        import test_chained_multi_window_gpu as M
        patch.setenv("WOFT_FUSED", "1")
        trk = M._two_motion_tracker([M._rect_mask(r) for r in (M.MASK_A, M.MASK_B, M.MASK_C)], **kw)
        assert trk._route == route and trk._margin, (trk._route, trk._margin)
        return _windowed(trk, [M.W._stub_frame(t) for t in range(1, 4)])
    return _private_pool(run)


SCENARIOS = {
    "full_bf16x3_otf": full_bf16x3_otf,
    "full_fp32": lambda patch: _one_flow(patch, iters=2, precision="fp32"),
    "full_bf16x3_volume": lambda patch: _one_flow(patch, iters=2, precision="bf16x3", corr="volume"),
    "small_bf16x3": lambda patch: _one_flow(patch, iters=3, precision="bf16x3", raft_type="orig", small=True,
                                            sd=dict(small=True, weighted=False)),
    "switches_off": switches_off,
    "full_fp16": lambda patch: _one_flow(patch, iters=2, precision="fp16"),
    "mask_head": mask_head,
    "generic_weight_head": lambda patch: _one_flow(patch, iters=2, precision="bf16x3", wh=[(64, 5), (32, 3)],
                                                   sd=dict(weight_head_structure=[(64, 5), (32, 3)])),
    "flow_region": flow_region,
    "tracker_wlsq": _tracker_scenario("WOFT.py", check=_is(_sparse_weights=True, _fused=True), lost_from=2),
    "tracker_irls": _tracker_scenario("WOFT_IRLS.py", check=_is(_fused=True)),
    "tracker_ransac": _tracker_scenario("WOFT_RANSAC.py", check=_is(_fused=True)),
    "tracker_trs": _tracker_scenario("WOFT_TRS.py", check=_is(_fused=True)),
    "tracker_visibility_gate": _tracker_scenario("WOFT_visibility.py", edit=_visibility_gate, mh=[(128, 3), (128, 3)],
                                                 check=_is(_fused=True, _vis_mode="gate")),
    "tracker_fbcheck": _tracker_scenario("WOFT_fbcheck.py", check=_is(_fused=True, fb_check="gate")),
    "tracker_nodraw": _tracker_scenario("WOFT.py", edit=_set(subsampler_fn=None), check=_is(_fused=True)),
    "tracker_callables": _tracker_scenario("WOFT.py", edit=_set(device_solver=False), check=_is(_fused=False)),
    "window_lost": _tracker_scenario("WOFT_window.py", edit=lambda conf: setattr(conf, "redet_success_fn", _never()),
                                     check=_is(_fused=True)),
    "chained": _chained_scenario(False),
    "chained_multi_batched": _chained_scenario(True, route="batched"),
    "chained_multi_select": lambda patch: _chained_scenario(True, route="select", estimator=_ransac())(patch),
    "chained_multi_loop": _chained_scenario(True, route="loop", subsampler_fn=None),
    "chained_window": _private_pool(_chained_window_scenario),
    "chained_multi_window_batched": _chained_multi_window_scenario("batched"),
    "chained_multi_window_select": lambda patch: _chained_multi_window_scenario("select", estimator=_ransac())(patch),
    "chained_multi_window_loop": _chained_multi_window_scenario("loop", subsampler_fn=None),
}


@torch.no_grad()
def run_scenario(name, patch):
    """-> (fixture lines of the scenario's trace, crc32 of its outputs).  patch: a pytest MonkeyPatch."""
    proxy = LibProxy(_lib.load())
    patch.setattr(_lib, "_lib", proxy)
    outs = SCENARIOS[name](patch)
    torch.cuda.synchronize()
    crc = 0
    for t in outs:
        if t is not None:
            crc = zlib.crc32(t.detach().cpu().contiguous().numpy().tobytes(), crc)
    return lines(proxy.calls), crc


def record(path=FIXTURE):
    """Every scenario twice; the output CRC is kept where the two runs agree (else null: not reproducible run to run)."""
    import pytest
    out = {}
    for name in SCENARIOS:
        runs = []
        for _ in range(2):
            with pytest.MonkeyPatch.context() as patch:
                runs.append(run_scenario(name, patch))
        diff = first_difference(runs[0][0], runs[1][0])
        if diff is not None:
            raise SystemExit(f"{name}: two runs of the same code differ at call {diff[0]}:\n  {diff[1]}\n  {diff[2]}")
        keep = runs[0][1] == runs[1][1]
        print(f"{name}: {len(runs[0][0])} calls, outputs {runs[0][1]:08x} / {runs[1][1]:08x}{'' if keep else '  (dropped)'}", flush=True)
        out[name] = {"out_crc": runs[0][1] if keep else None, "calls": runs[0][0]}
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=0) + "\n")


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        raise SystemExit("usage: python tests/launch_trace.py --record [fixture path]")
    record(Path(sys.argv[2]) if len(sys.argv) > 2 else FIXTURE)
