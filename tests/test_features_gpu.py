"""Frame-features records on the GPU: the pack / unpack launches against plain torch indexing on the same
buffers, flows from records against flows from images, stale-state scenarios, the error cases and the trackers with sharing on
against sharing off.  Every comparison is exact equality of bytes (floats compared as their int32 bit patterns, so NaNs count):
a restored state is produced by the same launch programs on the same input bits."""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from woft_amd import ops, synth  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
SIZES = [(128, 160), (136, 200)]          # 16 x 20 map: P = 320, 64 zero pad rows in f1rows; 17 x 25 map, odd both ways: P = 425
MASK_HEAD = [(64, 3)]
FULL, SMALL = (256, 128, 128, 256), (128, 96, 64, 160)      # fdim, hdim, cdim, channel stride of the GRU input buffer


def ibits(t):
    t = t.contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def same(a, b):
    """Two compute_flow results (tuples of tensors / None): the same structure, shapes and bytes."""
    a, b = (x if isinstance(x, (tuple, list)) else (x,) for x in (a, b))
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if (x is None) != (y is None):
            return False
        if x is not None and (x.shape != y.shape or x.dtype != y.dtype or not torch.equal(ibits(x), ibits(y))):
            return False
    return True


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------
SENT = -7.25


def _rand(rows, c, seed):
    """Seeded values with a few non-finite and denormal ones planted (a copy moves bits, whatever they are)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(rows, c, generator=g) * 3
    flat = t.view(-1).view(torch.int32)
    n = flat.numel()
    for k, v in enumerate((0x7FC00001, 0x7F800000, -0x00800000, 0x00000001, -0x7FFFFFFF - 1, 0x7FA12345 - 0x00A00000)):
        flat[(k * 7919 + seed) % n] = v
    return t.cuda()


@pytest.mark.parametrize("dims", [FULL, SMALL], ids=["full", "small"])
@pytest.mark.parametrize("P", [1, 63, 320, 425])
def test_pack_and_unpack_against_torch_indexing(P, dims):
    fdim, hdim, cdim, xcs = dims
    assert xcs > cdim
    rows = (P + 127) // 128 * 128
    f1rows = torch.zeros(rows, fdim, device="cuda")
    f1rows[:P] = _rand(P, fdim, 1)
    net, xbuf = _rand(P, hdim, 2), _rand(P, xcs, 3)
    record = torch.full((ops.features_record_floats(P, fdim, hdim, cdim),), SENT, device="cuda")
    ops.features_pack(f1rows, net, xbuf, P, (fdim, hdim, cdim), record)
    want = torch.cat([f1rows[:P].reshape(-1), net.reshape(-1), xbuf[:, :cdim].reshape(-1)])
    assert torch.equal(ibits(record), ibits(want))
    assert record.numel() * 4 == 4 * P * (fdim + hdim + cdim)

    # source role: every destination sits inside an arena of sentinels; f1rows / f1s have zero pad rows beyond P
    def arena(n_rows, c, dtype=torch.float32, zero_from=None):
        a = torch.full((n_rows + 16, c), SENT, dtype=dtype, device="cuda")
        if zero_from is not None:
            a[8 + zero_from:8 + n_rows] = 0
        return a, a[8:8 + n_rows]
    A_f, d_f = arena(rows, fdim, zero_from=P)
    A_s, d_s = arena(rows, 2 * fdim, dtype=torch.bfloat16, zero_from=P)
    A_n, d_n = arena(P, hdim)
    A_x, d_x = arena(P, xcs)
    A_i, d_i = arena(P, cdim)
    ops.features_unpack(record, P, (fdim, hdim, cdim), d_f, d_s, d_n, d_x, d_i)
    assert torch.equal(ibits(d_f[:P]), ibits(f1rows[:P])) and not d_f[P:].any()
    split = torch.full((rows, 2 * fdim), SENT, dtype=torch.bfloat16, device="cuda")
    ops.split_bf16_lines(f1rows, split)                               # the existing split step on the same (padded) rows
    assert torch.equal(ibits(d_s), ibits(split)) and not d_s[P:].view(torch.int16).any()
    assert torch.equal(ibits(d_n), ibits(net))
    assert torch.equal(ibits(d_x[:, :cdim]), ibits(xbuf[:, :cdim])) and (d_x[:, cdim:] == SENT).all()
    assert torch.equal(ibits(d_i), ibits(xbuf[:, :cdim]))
    for A, n_rows in ((A_f, rows), (A_s, rows), (A_n, P), (A_x, P), (A_i, P)):
        assert (A[:8] == SENT).all() and (A[8 + n_rows:] == SENT).all()
    # without the fused split the operand is left alone
    A_s2, d_s2 = arena(rows, 2 * fdim, dtype=torch.bfloat16)
    ops.features_unpack(record, P, (fdim, hdim, cdim), d_f, None, d_n, d_x, d_i)
    assert (A_s2 == SENT).all()

    # target role: the fnet map alone, into a map of its own inside an arena
    A_t, d_t = arena(P, fdim)
    ops.features_unpack(record, P, (fdim, hdim, cdim), d_t)
    assert torch.equal(ibits(d_t), ibits(f1rows[:P])) and (A_t[:8] == SENT).all() and (A_t[8 + P:] == SENT).all()


def _plan_tensors(plan):
    """Every device tensor a plan owns, by name (Acts by their rows)."""
    out = {}

    def visit(name, v):
        if isinstance(v, torch.Tensor) and v.is_cuda:
            out[name] = v
        elif isinstance(v, ops.Act):
            out[name] = v.t
        elif isinstance(v, (list, tuple)):
            for k, x in enumerate(v):
                visit(f"{name}[{k}]", x)
        elif isinstance(v, dict):
            for k, x in v.items():
                visit(f"{name}[{k!r}]", x)
    for name, v in vars(plan).items():
        if name != "eng":
            visit(name, v)
    return out


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
def test_unpack_writes_only_the_named_maps_of_a_plan(small):
    """On a real plan at 128 x 160, every buffer pre-filled with a sentinel (pad rows of f1rows / f1s with zeros)."""
    from woft_amd.engine import RaftEngine
    eng = RaftEngine(synth.make_state_dict(seed=3, small=small, weighted=not small), small=small, weighted=not small,
                     precision="bf16x3", corr="otf")
    plan = eng.plan(128, 160)
    P, (fdim, hdim, cdim) = plan.P, plan.record_dims
    assert P == 320 and plan.f1rows.shape[0] == 384 and plan.xbuf.cs > cdim
    record = _rand(1, ops.features_record_floats(P, fdim, hdim, cdim), 5).reshape(-1)
    tensors = _plan_tensors(plan)
    for t in tensors.values():
        if t.is_floating_point():
            t.fill_(SENT)
    plan.f1rows[P:] = 0
    plan.f1s[P:] = 0
    before = {n: t.clone() for n, t in tensors.items()}
    f_map, n_map, i_map = record[:P * fdim].view(P, fdim), record[P * fdim:P * (fdim + hdim)].view(P, hdim), \
        record[P * (fdim + hdim):].view(P, cdim)

    def check(written, role):
        """written: {buffer: expected}.  Those hold the expected bytes; every other tensor of the plan holds what it held (a view
        into a written buffer -- f1 into f1rows, flow_cat into xbuf -- is covered by the check of the buffer itself)."""
        exact = {(b.data_ptr(), tuple(b.shape)): e for b, e in written}
        storages = {b.untyped_storage().data_ptr() for b, _ in written}
        n_checked = 0
        for n, t in tensors.items():
            key = (t.data_ptr(), tuple(t.shape))
            if key in exact:
                assert torch.equal(ibits(t), ibits(exact[key])), f"{role}: {n}"
                n_checked += 1
            elif t.untyped_storage().data_ptr() not in storages:
                assert torch.equal(ibits(t), ibits(before[n])), f"{role} wrote {n}"
        assert n_checked >= len(written)

    ops.features_unpack(record, P, plan.record_dims, plan.f2act[0].t)                       # target role
    check([(plan.f2act[0].t, f_map)], "target role")

    plan.f2act[0].t.fill_(SENT)
    ops.features_unpack(record, P, plan.record_dims, plan.f1rows, plan.f1s, plan.net0.t, plan.xbuf.t, plan.inp_c.t)
    split = torch.zeros_like(plan.f1s)
    ops.split_bf16_lines(plan.f1rows, split)
    check([(plan.f1rows, torch.cat([f_map, torch.zeros(64, fdim, device="cuda")])), (plan.f1s, split), (plan.net0.t, n_map),
           (plan.inp_c.t, i_map), (plan.f2act[0].t, torch.full_like(f_map, SENT)),
           (plan.xbuf.t, torch.cat([i_map, torch.full((P, plan.xbuf.cs - cdim), SENT, device="cuda")], 1))], "source role")
    assert not plan.f1rows[P:].any() and not plan.f1s[P:].view(torch.int16).any()
    assert (plan.xbuf.t[:, cdim:] == SENT).all()


# ---- 2. flows from records ------------------------------------------------------------------------------------------------------------
def _config(raft_type="weighted", small=False, precision="bf16x3", corr="otf", iters=4, seed=7, graph=False, corr_band=None):
    from woft_amd.config import Config
    from woft_amd.flow_provider import RAFTWrapper
    masked = raft_type == "weighted_masked"
    c = Config()
    c.of_class = RAFTWrapper
    c.raft_type = raft_type
    c.class_params = Config()
    c.class_params.small = small
    c.class_params.mixed_precision = False
    c.class_params.alternate_corr = False
    c.class_params.weight_head_structure = [(128, 3)] * 3
    if masked:
        c.class_params.mask_estimation, c.class_params.mask_head_structure = True, MASK_HEAD
    c.model = synth.make_state_dict(seed=seed, small=small, weighted=raft_type != "orig",
                                    mask_head_structure=MASK_HEAD if masked else None)
    c.iters, c.padding_mode, c.precision, c.corr = iters, "RAFT", precision, corr
    if graph:
        c.graph = True
    if corr_band is not None:
        c.corr_band = corr_band
    return c


def _provider(**kw):
    c = _config(**kw)
    return c.of_class(c)


@pytest.fixture(scope="module")
def pairs():
    """Per size: two frames of a seeded texture (integer shift) and a third image; left unchanged."""
    out = {}
    for h, w in SIZES:
        big = synth.make_template(h + 32, w + 32, seq_id=9)
        out[(h, w)] = [np.ascontiguousarray(big[16 - t:16 - t + h, 16 + 2 * t:16 + 2 * t + w]) for t in (0, 1, 3)]
    return out


@pytest.mark.parametrize("precision,corr", [("bf16x3", "otf"), ("fp32", "otf"), ("bf16x3", "volume")])
@pytest.mark.parametrize("raft_type,small", [("orig", False), ("weighted", False), ("weighted_masked", False), ("weighted", True)])
def test_flows_from_records_have_the_bytes_of_flows_from_images(pairs, raft_type, small, precision, corr):
    prov = _provider(raft_type=raft_type, small=small, precision=precision, corr=corr)
    n_out = {"flow": 2, "TC": 3}
    for size in SIZES:
        a, b, _ = pairs[size]
        ref = {m: prov.compute_flow(a, b, mode=m) for m in ("flow", "TC")}
        for m in ref:
            assert len(ref[m]) == n_out[m] + (raft_type == "weighted_masked") and float(ref[m][0 if m == "flow" else 1].abs().max()) > 0
            assert (ref[m][n_out[m] - 1] is None) == (raft_type == "orig")
        ra, rb = prov.encode_frame(a), prov.encode_frame(b)
        assert ra.provider is prov and ra.shape == a.shape and ra.size == size and ra.geometry == (size[0], size[1], 0, 0)
        P = size[0] // 8 * (size[1] // 8)
        fdim, hdim, cdim = (128, 96, 64) if small else (256, 128, 128)
        assert ra.nbytes == 4 * P * (fdim + hdim + cdim) == ra.record.numel() * 4
        plan = prov.engine.plan(*size)
        own = {ra.record.untyped_storage().data_ptr(), rb.record.untyped_storage().data_ptr()}
        assert len(own) == 2 and not own & {t.untyped_storage().data_ptr() for t in _plan_tensors(plan).values()}
        for m in ("flow", "TC"):
            for src, dst, tag in ((ra, rb, "record/record"), (ra, b, "record/image"), (a, rb, "image/record")):
                assert same(prov.compute_flow(src, dst, mode=m), ref[m]), (size, m, tag)
    # the pinned image as source keeps the pinned fast path (buffer set 0, resident source) with a record as target
    for size in SIZES:
        a, b, _ = pairs[size]
        ref = {m: prov.compute_flow(a, b, mode=m) for m in ("flow", "TC")}
        prov.pin_source(a)
        rb = prov.encode_frame(b)
        for m in ("flow", "TC"):
            assert same(prov.compute_flow(a, rb, mode=m), ref[m]), (size, m, "pinned image/record")
            assert prov.last_flow_key[0] == 0 and prov.engine.plan(*size).source_tag is prov
        prov.pin_source(None)


def test_flow_init_iters_and_skip_weights_with_records(pairs):
    prov = _provider()
    size = SIZES[1]
    a, b, _ = pairs[size]
    init = torch.randn(2, size[0] // 8, size[1] // 8, generator=torch.Generator().manual_seed(4)).cuda()
    calls = [dict(flow_init=init), dict(iters=3), dict(skip_weights=True), dict(mode="TC", keep_flow=True, do_sigmoid=True)]
    refs = [prov.compute_flow(a, b, **dict(dict(mode="flow"), **kw)) for kw in calls]
    assert refs[2][1] is None and not same(refs[0], refs[1])
    ra, rb = prov.encode_frame(a), prov.encode_frame(b)
    for kw, ref in zip(calls, refs):
        assert same(prov.compute_flow(ra, rb, **dict(dict(mode="flow"), **kw)), ref), kw
    kept = prov.flow_map().clone()                                    # (the provider's buffer: the next call overwrites it)
    assert same(kept, prov.compute_flow(a, b, mode="flow", do_sigmoid=True)[0])


def test_graph_provider_alternating_images_and_records(pairs):
    prov = _provider(graph=True)
    assert prov.use_graph
    a, b, _ = pairs[SIZES[0]]
    ref = _provider().compute_flow(a, b, mode="flow")
    ra, rb = prov.encode_frame(a), prov.encode_frame(b)
    # (the second call with one signature captures, the third replays: both kinds of target get there)
    for k, (src, dst) in enumerate([(a, b), (ra, rb), (a, b), (ra, rb), (a, rb), (a, b), (ra, rb), (ra, b)]):
        assert same(prov.compute_flow(src, dst, mode="flow"), ref), k
    plan = prov.engine.plan(*SIZES[0])
    keys = [k for k, g in plan._graphs.items() if g is not None]
    assert {k.target_restored for k in keys} == {False, True}         # a captured graph for the encoded and for the restored target


# ---- 3. no stale state ----------------------------------------------------------------------------------------------------------------
def test_a_record_survives_intervening_work(pairs):
    prov = _provider()
    a, b, c = pairs[SIZES[0]]
    ref = prov.compute_flow(a, b, mode="TC")
    ref_ba = prov.compute_flow(b, a, mode="TC")
    ra, rb = prov.encode_frame(a), prov.encode_frame(b)
    keep = (ra.record.clone(), rb.record.clone())
    o1, o2, o3 = pairs[SIZES[1]]
    prov.compute_flow(o1, o2)                                         # the other size
    prov.pin_source(c)
    prov.compute_flow(c, a)                                           # a pinned template, both buffer sets in use
    prov.compute_flow(b, c)
    prov.weight_head_parameters()
    prov.sync_weight_head()                                           # an unchanged head: the records stay valid
    assert torch.equal(ibits(ra.record), ibits(keep[0])) and torch.equal(ibits(rb.record), ibits(keep[1]))
    assert same(prov.compute_flow(ra, rb, mode="TC"), ref)
    # one record as target, then as source
    assert same(prov.compute_flow(rb, ra, mode="TC"), ref_ba)
    assert same(prov.compute_flow(ra, rb, mode="TC"), ref)


def test_the_pinned_template_is_left_alone(pairs):
    a, b, c = pairs[SIZES[0]]
    fresh = _provider()
    fresh.pin_source(c)
    ref = fresh.compute_flow(c, a, mode="TC")
    prov = _provider()
    prov.pin_source(c)
    prov.compute_flow(c, b)
    plan0 = prov.engine.plan(*SIZES[0])
    resident = {n: t.clone() for n, t in (("f1rows", plan0.f1rows), ("f1s", plan0.f1s), ("net0", plan0.net0.t), ("inp_c", plan0.inp_c.t),
                                           ("gz", plan0.gate_bias[0][0].t), ("gq", plan0.gate_bias[0][1].t))}
    ra, rb = prov.encode_frame(a), prov.encode_frame(b)
    prov.compute_flow(ra, rb)
    prov.compute_flow(rb, a)
    for n, t in (("f1rows", plan0.f1rows), ("f1s", plan0.f1s), ("net0", plan0.net0.t), ("inp_c", plan0.inp_c.t),
                 ("gz", plan0.gate_bias[0][0].t), ("gq", plan0.gate_bias[0][1].t)):
        assert torch.equal(ibits(t), ibits(resident[n])), n
    assert plan0.source_tag is prov
    assert same(prov.compute_flow(c, a, mode="TC"), ref)
    assert same(prov.compute_flow(c, ra, mode="TC"), ref)


def test_src_is_previous_dst_finds_nothing_stale_after_a_record_flow(pairs):
    a, b, c = pairs[SIZES[0]]
    prov = _provider()
    ref = prov.compute_flow(b, c, mode="TC")
    # the honoured case first: b was the previous target, its features are reused
    prov.compute_flow(a, b)
    assert same(prov.compute_flow(b, c, mode="TC", src_is_previous_dst=True), ref) and prov.source_features_reused
    # a record flow in between replaces the target features: nothing may be reused
    for between in ("record target", "encode only"):
        prov.compute_flow(a, b)
        if between == "record target":
            prov.compute_flow(a, prov.encode_frame(c))
        else:
            prov.encode_frame(c)
        assert same(prov.compute_flow(b, c, mode="TC", src_is_previous_dst=True), ref), between
        assert not prov.source_features_reused, between


def test_replayed_and_eager_calls_leave_the_same_state(pairs):
    """A provider that replays hipGraphs and an eager one, driven through the same calls: after every call the same output bytes,
    the same source_features_reused / weights_deferred, and in both buffer sets the same band_valid, target_valid and source
    ownership -- a replay applies the state its flow() left.  3 iterations with corr_band=True: the band applies except under a
    warm start."""
    size = SIZES[0]
    a, b, c = pairs[size]
    eager, graph = _provider(iters=3, corr_band=True), _provider(iters=3, corr_band=True, graph=True)
    assert graph.use_graph and not eager.use_graph
    init = torch.randn(2, size[0] // 8, size[1] // 8, generator=torch.Generator().manual_seed(4)).cuda()
    pts = torch.tensor([[5.0, 7.0], [100.0, 90.0], [159.0, 127.0], [0.0, 0.0]], device="cuda")
    count = torch.tensor([4], dtype=torch.int32, device="cuda")
    rec = {}

    def encode(p):
        rec[p] = p.encode_frame(c)
        return rec[p].record

    def deferred(p):
        out = p.compute_flow(a, b, mode="TC", weight_region=True, defer_weights=4)
        assert p.weights_deferred and out[2] is None
        return out[:2] + (p.finish_weights(pts, count, 4, out=torch.zeros(4, device="cuda")),)

    def sync(p):
        p.weight_head_parameters()
        p.sync_weight_head()

    image = lambda p: p.compute_flow(a, b, mode="flow")
    steps = [("image/image", image)] * 3                                  # (the third call with one key replays)
    steps += [("sync_weight_head", sync)] + [("image/image after sync", image)] * 3        # (the graphs are dropped: captured again)
    steps += [("encode_frame", encode), ("image/image after encode_frame", image),
              ("src_is_previous_dst", lambda p: p.compute_flow(b, c, mode="TC", src_is_previous_dst=True)),
              ("record target", lambda p: p.compute_flow(a, rec[p], mode="flow")),
              ("record source", lambda p: p.compute_flow(rec[p], b, mode="flow"))]
    steps += [("flow_init", lambda p: p.compute_flow(a, b, mode="flow", flow_init=init))] * 3
    steps += [("deferred weights", deferred)] * 3
    steps += [("pin_source", lambda p: p.pin_source(a))]
    steps += [("pinned source", image), ("second buffer set", lambda p: p.compute_flow(b, c, mode="flow", skip_weights=True))] * 3
    steps += [("pinned source, resident", lambda p: p.compute_flow(a, c, mode="TC"))]
    for k, (name, call) in enumerate(steps):
        got, want = call(graph), call(eager)
        assert (got is None and want is None) or same(got, want), (k, name)
        assert (graph.source_features_reused, graph.weights_deferred) == (eager.source_features_reused, eager.weights_deferred), (k, name)
        for slot in (0, 1):
            pg, pe = graph.engine.plan(*size, slot), eager.engine.plan(*size, slot)
            state = lambda plan, p: (plan.band_valid, plan.target_valid, plan.source_tag is p)
            assert state(pg, graph) == state(pe, eager), (k, name, slot)
        if name == "src_is_previous_dst":                               # (the one intended change: True under a graph as it is eagerly)
            assert eager.source_features_reused and graph.source_features_reused
    captured = {key for slot in (0, 1) for key, g in graph.engine.plan(*size, slot)._graphs.items() if g is not None}
    assert len(captured) >= 3 and not any(eager.engine.plan(*size, slot)._graphs for slot in (0, 1))


def _reachable(root, found, seen):
    """Every object reachable from `root` through dicts, sequences and the attributes of woft_amd's own objects -> found."""
    if id(root) in seen or isinstance(root, (str, bytes, torch.Tensor, np.ndarray)):
        return
    seen.add(id(root))
    found.append(root)
    if isinstance(root, dict):
        children = list(root.keys()) + list(root.values())
    elif isinstance(root, (list, tuple, set, frozenset)):
        children = list(root)
    elif type(root).__module__.startswith("woft_amd") and hasattr(root, "__dict__"):
        children = list(vars(root).values())
    else:
        return
    for child in children:
        _reachable(child, found, seen)


def test_a_dropped_plan_leaves_nothing_behind():
    """bound_plans(1) over three shapes and back to the first: whatever the provider holds outside its engine refers to no plan
    the engine has dropped -- neither the plan nor its id() -- and every flow has the bytes of an unbounded provider's."""
    from woft_amd.engine import _Plan
    shapes = [(128, 160), (136, 200), (120, 152), (128, 160)]
    prov, ref = _provider(iters=3), _provider(iters=3)
    prov.bound_plans(1)
    plans = []                                                          # (kept alive here, so that no id() is handed out twice)
    for h, w in shapes:
        big = synth.make_template(h + 32, w + 32, seq_id=9)
        a, b, c = (np.ascontiguousarray(big[16 - t:16 - t + h, 16 + 2 * t:16 + 2 * t + w]) for t in (0, 1, 3))
        got, want = ((p.compute_flow(a, b, mode="flow"), p.compute_flow(b, c, mode="TC", src_is_previous_dst=True)) for p in (prov, ref))
        assert same(got[0], want[0]) and same(got[1], want[1]), (h, w)
        assert prov.source_features_reused and ref.source_features_reused
        plans.append(prov.engine.plan(h, w))
    live = list(prov.engine._plans.values())
    assert len(live) == 1 and live[0] is plans[3] and plans[3] is not plans[0] and len(ref.engine._plans) == 3
    dropped = plans[:3]
    held = []
    _reachable({k: v for k, v in vars(prov).items() if k != "engine"}, held, set())
    assert not [x for x in held if isinstance(x, _Plan) and x is not live[0]]
    assert not [x for x in held if isinstance(x, int) and not isinstance(x, bool) and x in {id(p) for p in dropped}]


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_reason(pairs):
    prov, other = _provider(), _provider(raft_type="orig")
    a, b, _ = pairs[SIZES[0]]
    big = pairs[SIZES[1]][0]
    ra = prov.encode_frame(a)
    with pytest.raises(ValueError, match="geometr"):
        prov.compute_flow(ra, prov.encode_frame(big))
    with pytest.raises(ValueError, match="geometr"):
        prov.compute_flow(big, ra)
    with pytest.raises(ValueError, match="another provider"):
        prov.compute_flow(other.encode_frame(a), b)
    with pytest.raises(ValueError, match="another provider"):
        other.compute_flow(a, ra)
    with pytest.raises(ValueError, match="src_img_identifier"):
        prov.compute_flow(ra, b, src_img_identifier=("d", "s", 0))
    with pytest.raises(TypeError, match="uint8"):
        prov.encode_frame(a.astype(np.float32))


# ---- 5. the trackers ------------------------------------------------------------------------------------------------------------------
FIELDS = ("flow", "cost", "vis", "occluded", "sel")


@pytest.mark.parametrize("raft_type", ["weighted", "weighted_masked"])
def test_multiflowtracker_with_sharing_on_and_off(raft_type):
    from woft_amd import MultiFlowTracker
    h, w = SIZES[0]
    big = synth.make_template(h + 32, w + 32, seq_id=9)
    frames = [np.ascontiguousarray(big[16 - t:16 - t + h, 16 + 2 * t:16 + 2 * t + w]) for t in range(7)]
    outs = {}
    for share in (False, True):
        trk = MultiFlowTracker(_provider(raft_type=raft_type), deltas=(None, 1, 2, 4), iters=4, share_features=share)
        trk.init(frames[0])
        outs[share] = [trk.track(f) for f in frames[1:]]
        assert sorted(trk._records) == (sorted(trk._ring) if share else [])
    wins = set()
    for t, (x, y) in enumerate(zip(outs[False], outs[True]), 1):
        assert x.frame_index == y.frame_index == t
        for n in FIELDS:
            assert torch.equal(ibits(getattr(x, n)), ibits(getattr(y, n))), (t, n)
        wins |= set(torch.unique(x.sel).tolist())
    assert len(wins - {-1}) >= 1 and float(outs[False][-1].flow.nan_to_num().abs().max()) > 0


def test_compute_flow_fb_with_shared_features(pairs):
    prov = _provider()
    a, b, _ = pairs[SIZES[1]]
    ref = prov.compute_flow_fb(a, b)
    assert same(prov.compute_flow_fb(a, b, share_features=True), ref)
    assert same(prov.compute_flow_fb(prov.encode_frame(a), b, share_features=True), ref)
    assert same(prov.compute_flow_fb(prov.encode_frame(a), prov.encode_frame(b)), ref)
    assert 0 < float(ref[3].mean()) <= 1


def test_woft_chained_shared_against_woft_chained():
    from pytracking.utils.config import load_config
    h, w = SIZES[0]
    big = synth.make_template(h + 32, w + 32, seq_id=5)
    frames = [np.ascontiguousarray(big[16 - t:16 - t + h, 16 + 2 * t:16 + 2 * t + w]) for t in range(6)]
    mask = synth.make_init_mask(h, w)
    runs = {}
    for name in ("WOFT_chained.py", "WOFT_chained_shared.py"):
        conf = load_config(ROOT / "pytracking" / "configs" / name)
        fc = conf.flow_config
        fc.model, fc.iters, fc.precision = synth.make_state_dict(seed=7), 4, "bf16x3"
        conf.chain_deltas = (None, 1, 2)
        trk = conf.tracker_class(conf)
        assert trk.multi.share_features == (name == "WOFT_chained_shared.py")
        trk.init(frames[0], mask)
        runs[name] = [trk.track(f) for f in frames[1:]]
        assert sorted(trk.multi._records) == (sorted(trk.multi._ring) if trk.multi.share_features else [])
    assert len(runs["WOFT_chained.py"]) == 5
    for t, ((Ha, ma), (Hb, mb)) in enumerate(zip(*runs.values()), 1):
        assert np.array_equal(np.asarray(Ha).view(np.uint64), np.asarray(Hb).view(np.uint64)), t
        chain = sorted(k for k in vars(ma) if k.startswith("chain_"))
        assert chain == sorted(k for k in vars(mb) if k.startswith("chain_")) and {"chain_hist", "chain_invalid", "chain_occluded"} <= set(chain)
        for k in chain:
            assert np.array_equal(np.asarray(getattr(ma, k)), np.asarray(getattr(mb, k))), (t, k)
        assert (ma.lost, ma.n_kept) == (mb.lost, mb.n_kept)
