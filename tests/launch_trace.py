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
            self.calls.append((name, [self._value(t, a) for t, a in zip(sig[1], args)], _summary(args)))
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
