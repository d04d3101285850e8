"""The grid of ops.conv_params calls behind tests/golden/conv_select.npz (helper of test_conv_select_cpu.py, not collected).

conv_params only reads its operands' geometry and addresses: with ops.DEV = "cpu" it runs on host tensors and never loads the
library.  The grid crosses every distinct conv of the full network, the small network, a mask head and a generic weight head (as
the engine packs them: strides, flat packing, the GRU's channel layouts) with map sizes, precisions and option sets; on the plain
option set every switch is also flipped alone.  A row of the fixture is the call's outcome (kernel, tiles, launched cout_pad,
effective precision and in_norm, _m_tiles, _m, which weight forms are set) plus the CRC32 of the whole struct in the canonical
form of tests/launch_trace.py (pointers numbered by first appearance: operands are distinct one-element tensors, so aliasing
shows), or the type of the exception the call raised.  The fixture also holds ops.pair_ok's verdict for every ordered pair of
layers within each (map, precision) group of the plain set.

The fixture is a record of the commit BEFORE a change of the selection (`python tests/conv_select_cases.py --record` there): a
refactor passes against it unchanged; a change that moves a rule on purpose re-records it.  Only ops.pack_conv, ops.Act,
ops.conv_params, ops.pair_ok, the switch attributes of ops and WOFT_MX_ZR are used, so that it runs at either commit.
"""
import json
import operator
import os
import re
import sys
import zlib
from contextlib import contextmanager
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for _p in (str(ROOT), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from launch_trace import LibProxy  # noqa: E402
from woft_amd import _lib, ops, synth  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "conv_select.npz"
PRECISIONS = ("fp32", "bf16x3", "bf16", "fp16", "f16mx8")
HALOS = (0, 1, 2, 4, 7, 8, 12, 16)
# padded frame sizes: 128x160, 256x320, 480p, 720p, 1080p, 4K -> their 1/8-resolution maps, and the x2 / x4 encoder maps of each
FRAMES = ((128, 160), (256, 320), (480, 640), (720, 1280), (1088, 1920), (2160, 3840))
MAPS = [(1, h // d, w // d) for h, w in FRAMES for d in (8, 4, 2)] + [(1, 5, 12)]                    # (the last: smaller than a tile)
MAPS += [(n, s, s) for s in (9, 7) for n in (300, 1024, 4800)]                                       # weight-head windows
# maps that also run the non-plain option sets and the switches: a small and a large 1/8 map, an encoder map, the tiny one, windows
OPTION_MAPS = ((1, 16, 20), (1, 136, 240), (1, 64, 80), (1, 5, 12), (1024, 9, 9), (300, 7, 7))
# (attribute of ops | "WOFT_MX_ZR", value): each flipped alone on the plain option set
SWITCHES = (("USE_HALO", False), ("USE_REGB", False), ("REGB_TY4", False), ("USE_STEM", False), ("USE_1X1", False),
            ("WH_HALO", 1), ("HALO_MIN_BLOCKS", 100), ("TILE_MIN_BLOCKS", 100), ("MX_LAYERS", "all"), ("SLOW_GATES", True),
            ("WOFT_MX_ZR", "64"), ("WOFT_MX_ZR", "128"))
OPTIONS = (("plain", None), ("stats", None), ("in_norm", 1), ("in_norm", 2), ("x2", None), ("bias_map", None), ("wh0", None),
           ("flowhead", None), ("cout", None), ("tiles", (64, 64)), ("tiles", (128, 128))) + tuple(("halo", k) for k in HALOS)
OUTCOME = ("kernel", "tile_m", "tile_n", "cout_pad", "precision", "in_norm", "m_tiles", "m", "weights", "crc", "raised")


class Case(NamedTuple):
    layer: int          # index into layers()
    map: int            # index into MAPS
    precision: str
    option: tuple       # entry of OPTIONS
    switch: tuple       # entry of SWITCHES, or None


def layers():
    """-> [(name, PackedConv)]: the distinct convs (by everything conv_params reads of a PackedConv) of the networks, zero weights."""
    specs = []          # (name, OIHW shape, pack_conv keywords)

    def encoder(sd, p, small, split):
        specs.append((p + ".conv1", sd[p + ".conv1.weight"].shape, dict(stride=2, flat_cs=4)))
        for k in sd:
            m = re.fullmatch(rf"{p}\.layer(\d)\.(\d)\.(conv(\d)|downsample\.0)\.weight", k)
            if m:
                s = (1, 2, 2)[int(m[1]) - 1] if m[2] == "0" else 1
                strided = m[3].startswith("down") or m[4] == ("2" if small else "1")
                specs.append((k[:-7], sd[k].shape, dict(stride=s if strided else 1)))
        co, ci = sd[p + ".conv2.weight"].shape[:2]
        specs.extend((f"{p}.conv2[{a}:{b}]", (b - a, ci, 1, 1), {}) for a, b in split(co))

    def head(sd, prefix, flat0):
        idx = sorted(int(k.split(".")[2]) for k in sd if k.startswith(prefix) and k.endswith(".weight"))
        for j, i in enumerate(idx[:-1]):
            sh = sd[f"{prefix}{i}.weight"].shape
            specs.append((f"{prefix}{i}", sh, dict(flat_cs=8) if j == 0 and flat0 and sh[2] * 8 <= 32 else {}))

    for small, kw in ((False, dict(mask_head_structure=[(64, 3)])), (True, dict(weighted=False)),
                      (False, dict(weight_head_structure=[(64, 5), (32, 3)]))):
        sd = synth.make_state_dict(seed=0, small=small, **kw)
        hd, cd, mot = (96, 64, 82) if small else (128, 128, 128)
        encoder(sd, "fnet", small, lambda co: [(0, co)])
        encoder(sd, "cnet", small, lambda co: [(0, hd), (hd, co)])
        u = "update_block."
        for n in ("encoder.convc1", "encoder.convc2", "encoder.convf1", "encoder.convf2", "encoder.conv", "flow_head.conv1",
                  "flow_head.conv2", "mask.0", "mask.2"):
            if u + n + ".weight" in sd:
                specs.append((u + n, sd[u + n + ".weight"].shape, dict(flat_cs=4) if n == "encoder.convf1" else {}))
        dyn, ctx = [(0, hd, 0), (hd + cd, hd + cd + mot, hd)], [(hd, hd + cd, 0)]
        for sfx, pd in (("", None),) if small else (("1", (0, 2)), ("2", (2, 0))):
            co, ci, kh, kw_ = sd[f"{u}gru.convq{sfx}.weight"].shape
            for gates, c in (("zr", 2 * co), ("q", co)):
                specs.append((f"{u}gru.{gates}{sfx}.dyn", (c, ci, kh, kw_), dict(padding=pd, cin_layout=dyn)))
                specs.append((f"{u}gru.{gates}{sfx}.inp", (c, ci, kh, kw_), dict(padding=pd, cin_layout=ctx)))
        head(sd, "weight_head.net.", True)
        head(sd, "mask_head.net.", False)
    out, seen = [], set()
    dev, ops.DEV = ops.DEV, "cpu"
    try:
        for name, shape, kw in specs:
            key = (tuple(shape), tuple(sorted((k, str(v)) for k, v in kw.items())))
            if key not in seen:
                seen.add(key)
                out.append((name, ops.pack_conv(torch.zeros(*shape), None, **kw)))
    finally:
        ops.DEV = dev
    return out


def cases(n_layers):
    """Every layer x every map x every precision on the plain set; the other option sets and the switches on OPTION_MAPS (the
    thresholds are a matter of sizes, the eligibility rules one of flags: the full product would be a quarter of a million rows)."""
    for li in range(n_layers):
        for mi in range(len(MAPS)):
            for prec in PRECISIONS:
                yield Case(li, mi, prec, OPTIONS[0], None)
                if MAPS[mi] in OPTION_MAPS:
                    for opt in OPTIONS[1:]:
                        yield Case(li, mi, prec, opt, None)
                    for sw in SWITCHES:
                        yield Case(li, mi, prec, OPTIONS[0], sw)


_ONES = {}


def _one(role, *shape, dtype=torch.float32):
    """The operand `role`'s tensor of that shape on ONE element of its own: a distinct non-NULL address per role (an empty
    tensor's would be NULL and hide aliasing)."""
    key = (role,) + shape
    if key not in _ONES:
        _ONES[key] = torch.zeros(1, dtype=dtype).expand(*shape)
    return _ONES[key]


def call_args(case, pc):
    """-> (x, out, keywords) of the conv_params call of a case."""
    n, h, w = MAPS[case.map]
    x = ops.Act(_one("x", 1, pc.flat_cs if pc.flat else pc.cin_pad), n, h, w, pc.cin_pad)
    ho, wo = pc.out_hw(h, w)
    out = ops.Act(_one("out", 1, ops._round_up(pc.cout, 4)), n, ho, wo, pc.cout)
    kw = dict(precision=case.precision)
    name, val = case.option
    if name == "stats":
        kw["stats"] = (_one("sum", 1 << 30), _one("sq", 1 << 30))
    elif name == "in_norm":
        kw.update(in_norm=val, in_stats=(_one("mean", 256), _one("rstd", 256)))
    elif name == "x2":
        kw.update(x2=ops.Act(_one("x2", 1, max(pc.cin_pad - 32, 32)), n, h, w, pc.cin_pad - 32), c_split=32, x2_off=4)
    elif name == "bias_map":
        kw["bias_map"] = ops.Act(_one("bias_map", 1, ops._round_up(pc.cout, 4)), n, ho, wo, pc.cout)
    elif name == "wh0":
        kw["wh0"] = (ops.Act(_one("lookup", 1, 352), 1, 1, n, 324), _one("wmean", n), _one("wh0_w", 8), _one("wh0_b", 128),
                     _one("index", n, dtype=torch.int32))
    elif name == "flowhead":
        kw["epi"] = _lib.EPI_FLOWHEAD
    elif name == "cout":
        kw["cout"] = (pc.cout + 1) // 2
    elif name != "plain":
        kw[name] = val
    return x, out, kw


@contextmanager
def switched(sw):
    """One switch flipped for the duration of the block: an attribute of ops, or WOFT_MX_ZR in the environment."""
    env, saved = os.environ.pop("WOFT_MX_ZR", None), None
    try:
        if sw is not None and sw[0] == "WOFT_MX_ZR":
            os.environ["WOFT_MX_ZR"] = sw[1]
        elif sw is not None:
            saved = getattr(ops, sw[0])
            setattr(ops, sw[0], sw[1])
        yield
    finally:
        os.environ.pop("WOFT_MX_ZR", None)
        if env is not None:
            os.environ["WOFT_MX_ZR"] = env
        if saved is not None:
            setattr(ops, sw[0], saved)


_NAMES = [name for name, _ in _lib.ConvParams._fields_]
_FIELDS = operator.attrgetter(*_NAMES)
_POINTERS = [k for k, (_, t) in enumerate(_lib.ConvParams._fields_) if t is _lib.vp]
_FLOATS = [k for k, (_, t) in enumerate(_lib.ConvParams._fields_) if t is _lib.f32]
_ORDER = sorted(range(len(_NAMES)), key=_NAMES.__getitem__)
_FORMAT = "{" + ", ".join(f'"{_NAMES[k]}": %s' for k in _ORDER) + "}"


def canonical(p):
    """json.dumps(LibProxy(None)._struct(p), sort_keys=True) of a woft_conv_params, several times faster (a grid of tens of
    thousands of structs; test_conv_select_cpu.py checks the two against each other on a sample)."""
    v, ids = list(_FIELDS(p)), {}
    for k in _POINTERS:                                          # (numbered by first appearance in the struct's field order)
        v[k] = 0 if not v[k] else ids.setdefault(v[k], len(ids) + 1)
    for k in _FLOATS:
        v[k] = f'"{v[k].hex()}"'
    return _FORMAT % tuple(v[k] for k in _ORDER)


def canonical_reference(p):
    return json.dumps(LibProxy(None)._struct(p), sort_keys=True)


def outcome(p):
    """The fixture's row of a filled struct."""
    weights = bool(p.wgt_frag) | bool(p.wgt_mx) << 1 | bool(p.wgt_hi) << 2 | bool(p.wgt_lo) << 3
    return (p.halo, p.tile_m, p.tile_n, p.cout_pad, p.precision, p.in_norm, p._m_tiles, p._m, weights,
            zlib.crc32(canonical(p).encode()), 0)


def run(all_layers, raised, visit=None):
    """Every case -> (rows: int64 (cases, len(OUTCOME)), pairs: ops.pair_ok's verdict for every ordered pair of layers within each
    (map, precision) group of the plain set, a flat uint8 array).  raised: the list of exception type names a row's last column
    indexes (1-based), extended as new ones occur.  visit(case number, case, struct): called for every call that returned."""
    rows, pairs, plain = [], [], {}
    dev, ops.DEV = ops.DEV, "cpu"
    try:
        for k, case in enumerate(cases(len(all_layers))):
            pc = all_layers[case.layer][1]
            with switched(case.switch):
                try:
                    x, out, kw = call_args(case, pc)
                    p = ops.conv_params(x, pc, out, **kw)
                    rows.append(outcome(p))
                    if visit is not None:
                        visit(k, case, p)
                except Exception as e:                          # noqa: BLE001  (recorded: the call must keep raising it)
                    p, name = None, type(e).__name__
                    if name not in raised:
                        raised.append(name)
                    rows.append((0,) * (len(OUTCOME) - 1) + (raised.index(name) + 1,))
            if case.option == OPTIONS[0] and case.switch is None:
                plain[(case.map, case.precision, case.layer)] = p
        for mi in range(len(MAPS)):
            for prec in PRECISIONS:
                group = [plain[(mi, prec, li)] for li in range(len(all_layers))]
                pairs.extend(int(a is not None and b is not None and bool(ops.pair_ok(a, b))) for a in group for b in group)
    finally:
        ops.DEV = dev
    return np.array(rows, dtype=np.int64), np.array(pairs, dtype=np.uint8)


def record(path=FIXTURE):
    raised = []
    rows, pairs = run(layers(), raised)
    path.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(path, rows=rows.astype(np.uint32 if rows.min() >= 0 and rows.max() < 2 ** 32 else np.int64),
                        pairs=np.packbits(pairs), n_pairs=np.int64(pairs.size), raised=np.array(raised))
    print(f"{len(rows)} rows, {len(np.unique(rows[:, :9], axis=0))} distinct outcomes, {pairs.size} pairs ({int(pairs.sum())} ok), "
          f"raised: {raised}, {path.stat().st_size} bytes")


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        raise SystemExit("usage: python tests/conv_select_cases.py --record [fixture path]")
    record(Path(sys.argv[2]) if len(sys.argv) > 2 else FIXTURE)
