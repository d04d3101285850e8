"""Which part of the 1/8-resolution map each launch of the refinement loop has to compute when the caller reads the flow
only inside a rectangle (the tracker: its template mask, TRK:287-312).

Every layer of the update block (update.py:71-136) is a small convolution, so what a consumer reads of a producer's output is the
consumer's own output region grown by the consumer's taps.  Walking the launches of a whole flow BACKWARDS from what the caller
reads after the last iteration -- the convex upsampling's 3x3 support of the coordinates and its mask channels (weighted_raft.py:
92-103) -- gives every launch the rectangle it must produce; going backwards the rectangles grow (by 11 cells per iteration for
the full model) until they are the whole map, and from there on the launches are today's.  Nothing here is a constant of one
model: the growth comes from the kernel sizes of the layers themselves (`taps_of_state_dict`, or the engine's packed layers).

Pure Python, no torch and no device: the engine (woft_amd/engine.py: _Plan.set_flow_region) turns the rectangles into restricted
launches; tests/test_flow_region_cpu.py pins them against the CPU oracle.

A rectangle is (y0, x0, h, w) in cells; None = nothing is needed.
"""


def clip(rect, hf, wf):
    if rect is None:
        return None
    y0, x0, y1, x1 = max(rect[0], 0), max(rect[1], 0), min(rect[0] + rect[2], hf), min(rect[1] + rect[3], wf)
    return (y0, x0, y1 - y0, x1 - x0) if y1 > y0 and x1 > x0 else None


def dilate(rect, ry, rx, hf, wf):
    """rect grown by ry rows and rx columns on each side, clipped to the hf x wf map."""
    if rect is None:
        return None
    return clip((rect[0] - ry, rect[1] - rx, rect[2] + 2 * ry, rect[3] + 2 * rx), hf, wf)


def union(a, b):
    """Bounding rectangle of two rectangles."""
    if a is None or b is None:
        return a if b is None else b
    y0, x0 = min(a[0], b[0]), min(a[1], b[1])
    y1, x1 = max(a[0] + a[2], b[0] + b[2]), max(a[1] + a[3], b[1] + b[3])
    return (y0, x0, y1 - y0, x1 - x0)


def is_full(rect, hf, wf):
    return rect is not None and tuple(rect) == (0, 0, hf, wf)


def reach(kernel, pad):
    """How far a conv with `kernel` taps and zero padding `pad` along one axis reads beyond an output position (either side)."""
    return max(pad, kernel - 1 - pad)


# ---- the update block's layers ---------------------------------------------------------------------------------------------
# taps: {layer: (ry, rx)} = reach of each layer along y and x.  Layers of the full model (BasicUpdateBlock, update.py:82-136):
FULL_LAYERS = {"convc1": "update_block.encoder.convc1", "convc2": "update_block.encoder.convc2",
               "convf1": "update_block.encoder.convf1", "convf2": "update_block.encoder.convf2",
               "convm": "update_block.encoder.conv", "gru0": "update_block.gru.convz1", "gru1": "update_block.gru.convz2",
               "fh1": "update_block.flow_head.conv1", "fh2": "update_block.flow_head.conv2",
               "mk1": "update_block.mask.0", "mk2": "update_block.mask.2"}


def taps_of_state_dict(shape_of):
    """{layer: (ry, rx)} of the full model from the kernel sizes in a state dict; shape_of(name) -> the shape of `name`.weight.
    Every layer pads by half its kernel (update.py:9-11,36-42,82-86,118-125)."""
    out = {}
    for layer, name in FULL_LAYERS.items():
        kh, kw = shape_of(name)[2:]
        out[layer] = (reach(kh, kh // 2), reach(kw, kw // 2))
    return out


def iteration_launches(taps, first=False, last=False, folded=True):
    """The launches of ONE refinement iteration of the full model in execution order (engine._Plan._iter_program), as
    [(tag, [part, ...])], part = (layer, reads, writes), reads = [(buffer, ry, rx)].  A launch of two parts is a pair launch (or the
    lookup launch with the previous iteration's flow-head gather folded in): every part has a rectangle of its own.
    Buffers: coords, flow (the flow operand: flow4 and the flow channels of the GRU input), corr, c1, fl1, cf_c, cf_f, mot (the motion
    features), z, rh, net0 / hA / hB (GRU states), fh_part (the flow head's per-tap partial products), mk, mask."""
    h_in = "net0" if first else "hB"
    t = taps
    look = []
    if folded and not first:
        look.append(("gather", [("fh_part",) + t["fh2"], ("coords", 0, 0)], ["coords", "flow"]))
    look.append(("lookup", [("coords", 0, 0)], ["corr"]))
    x = lambda l: [("mot",) + t[l], ("flow",) + t[l]]
    out = [("lookup", look),
           ("convc1+convf1", [("convc1", [("corr",) + t["convc1"]], ["c1"]), ("convf1", [("flow",) + t["convf1"]], ["fl1"])]),
           ("convc2+convf2", [("convc2", [("c1",) + t["convc2"]], ["cf_c"]), ("convf2", [("fl1",) + t["convf2"]], ["cf_f"])]),
           ("convm", [("convm", [("cf_c",) + t["convm"], ("cf_f",) + t["convm"]], ["mot"])]),
           ("gru_zr0", [("gru_zr0", [(h_in,) + t["gru0"]] + x("gru0"), ["z", "rh"])]),
           ("gru_q0", [("gru_q0", [("rh",) + t["gru0"]] + x("gru0") + [(h_in, 0, 0), ("z", 0, 0)], ["hA"])]),
           ("gru_zr1", [("gru_zr1", [("hA",) + t["gru1"]] + x("gru1"), ["z", "rh"])]),
           ("gru_q1", [("gru_q1", [("rh",) + t["gru1"]] + x("gru1") + [("hA", 0, 0), ("z", 0, 0)], ["hB"])])]
    fh1 = ("fh1", [("hB",) + t["fh1"]], ["fh_part"])
    if last:
        out.append(("fh1+mk1", [fh1, ("mk1", [("hB",) + t["mk1"]], ["mk"])]))
    else:
        out.append(("fh1", [fh1]))
    return out


def closing_launches(taps):
    """After the last iteration: its flow-head gather as a launch of its own, then the mask head's second conv."""
    return [("fh_gather", [("gather", [("fh_part",) + taps["fh2"], ("coords", 0, 0)], ["coords", "flow"])]),
            ("mk2", [("mk2", [("mk",) + taps["mk2"]], ["mask"])])]


def flow_launches(taps, iters, folded=True):
    """Every launch of a flow of `iters` iterations: [(iteration | -1 for the closing launches, tag, parts)]."""
    out = []
    for it in range(iters):
        for tag, parts in iteration_launches(taps, first=it == 0, last=(it == iters - 1 and iters > 1), folded=folded):
            out.append((it, tag, parts))
        if not folded:
            out.append((it, "fh_gather", closing_launches(taps)[0][1]))
    tail = closing_launches(taps)
    if iters == 1:      # (a single iteration has no paired last launch: the mask head's first conv runs on its own)
        out.append((-1, "mk1", [("mk1", [("hB",) + taps["mk1"]], ["mk"])]))
    out += [(-1, tag, parts) for tag, parts in (tail if folded else tail[1:])]
    return out


def final_need(rect, hf, wf, up=1):
    """What the caller reads after the last iteration when it reads full-resolution flow only in the cells of `rect`: the convex
    upsampling combines the coordinates of the 3x3 neighbourhood (`up` = 1 cell) with the cell's own mask channels."""
    return {"coords": dilate(rect, up, up, hf, wf), "mask": clip(rect, hf, wf)}


def schedule(launches, need, hf, wf):
    """Walk `launches` (flow_launches) backwards from `need` ({buffer: rectangle read after the last launch}).
    -> ([[rect of each part] per launch], {buffer: rectangle read of it before the first launch}).
    A part's rectangle is the bounding rectangle of what later launches read of its outputs (None: nobody reads them): what it
    must produce.  A launch may always produce more -- a kernel that cannot be restricted runs on the whole map, and what it
    writes outside its rectangle, from inputs nobody vouches for, is never read."""
    need = dict(need)
    rects = [None] * len(launches)
    for k in range(len(launches) - 1, -1, -1):
        parts = launches[k][2]
        mine = [None] * len(parts)
        for j in range(len(parts) - 1, -1, -1):            # (the parts of a launch in their order: gather, then lookup)
            name, reads, writes = parts[j]
            out = None
            for w in writes:
                out = union(out, need.get(w))
                need[w] = None                              # produced here: what the buffer held before is not read
            mine[j] = out
            for buf, ry, rx in reads:
                need[buf] = union(need.get(buf), dilate(out, ry, rx, hf, wf))
        rects[k] = mine
    return rects, need


def step_margins(taps):
    """Cells of net_i / coords_i around a point that ONE iteration's outputs at that point depend on:
    {"net": (net_i margin, coords_i margin), "coords": (net_i margin, coords_i margin)} along (y, x) each -- the table of DESIGN
    section 4, derived and not stated."""
    big = 4096
    launches = [(1, tag, parts) for tag, parts in iteration_launches(taps, folded=False)]
    launches.append((1, "fh_gather", closing_launches(taps)[0][1]))
    c = big // 2
    out = {}
    for what, buf in (("net", "hB"), ("coords", "coords")):
        _, need = schedule(launches, {buf: (c, c, 1, 1)}, big, big)
        m = {}
        for src in ("hB", "coords"):
            r = need.get(src)
            if src == "coords":                             # (the flow operand is coords_i - grid: the same state)
                r = union(r, need.get("flow"))
            m[src] = (c - r[0], c - r[1]) if r is not None else (0, 0)
        out[what] = (m["hB"], m["coords"])
    return out
