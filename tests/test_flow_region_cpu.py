"""The dependency cone of one refinement iteration, pinned against the CPU oracle (oracle/raft_ref.py) and not against the code
that uses it: woft_amd/flow_region.py derives, from the kernel sizes in the state dict, how far around a point the iteration's
outputs read its input state; here the oracle's update step is run on a state perturbed OUTSIDE a box grown by those margins --
the outputs inside the box must not change at all -- and with any one margin one cell smaller, where they must."""
import pytest
import torch

from oracle import raft_ref
from woft_amd import flow_region, synth

HF, WF = 40, 56
BOX = (16, 22, 6, 9)            # (y0, x0, h, w): further than every margin from every border


@pytest.fixture(scope="module")
def model():
    sd = {k: v.float() for k, v in synth.make_state_dict(seed=3).items()}
    taps = flow_region.taps_of_state_dict(lambda name: tuple(sd[name + ".weight"].shape))
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    fmap1, fmap2 = r(1, 256, HF, WF), r(1, 256, HF, WF)
    state = dict(net=torch.tanh(r(1, 128, HF, WF)), coords=raft_ref.coords_grid(1, HF, WF) + 2.0 * r(1, 2, HF, WF))
    inp = torch.relu(r(1, 128, HF, WF))
    pyr = raft_ref.corr_pyramid(fmap1, fmap2)

    def step(net, coords):
        corr = raft_ref.corr_lookup(pyr, coords, 4)
        net1, _, delta = raft_ref.update_block(sd, net, inp, corr, coords - raft_ref.coords_grid(1, HF, WF), small=False)
        return dict(net=net1, coords=coords + delta)
    with torch.no_grad():
        ref = step(**state)
    return taps, state, step, ref, r


def test_margins_of_the_full_model(model):
    taps = model[0]
    m = flow_region.step_margins(taps)
    # GRU 1x5 / 5x1 twice = 4; + motion encoder conv 1, convf2 1, convf1 3 = 9; the flow head's two 3x3 convs add 2
    assert m == {"net": ((4, 4), (9, 9)), "coords": ((6, 6), (11, 11))}
    assert max(max(v) for pair in m.values() for v in pair) < min(BOX[0], BOX[1], HF - BOX[0] - BOX[2], WF - BOX[1] - BOX[3])


def _perturbed(state, noise, margins):
    """The state with noise added outside BOX grown by margins = {"net": (my, mx), "coords": (my, mx)}."""
    out = {}
    for key, t in state.items():
        my, mx = margins[key]
        keep = torch.zeros(1, 1, HF, WF, dtype=torch.bool)
        keep[..., BOX[0] - my:BOX[0] + BOX[2] + my, BOX[1] - mx:BOX[1] + BOX[3] + mx] = True
        out[key] = torch.where(keep, t, t + noise[key])
    return out


@pytest.mark.parametrize("what", ["net", "coords"])
def test_outputs_inside_the_box_depend_on_exactly_the_derived_margins(model, what):
    taps, state, step, ref, r = model
    m = flow_region.step_margins(taps)[what]
    margins = {"net": m[0], "coords": m[1]}
    noise = {"net": 0.5 * r(1, 128, HF, WF), "coords": 1.5 * r(1, 2, HF, WF)}
    inside = (Ellipsis, slice(BOX[0], BOX[0] + BOX[2]), slice(BOX[1], BOX[1] + BOX[3]))
    with torch.no_grad():
        got = step(**_perturbed(state, noise, margins))
        assert float((got[what][inside] - ref[what][inside]).abs().max()) == 0.0
        assert float((got[what] - ref[what]).abs().max()) > 0.0            # (the perturbation does reach the outputs elsewhere)
        for key in ("net", "coords"):
            for axis in (0, 1):
                less = dict(margins)
                less[key] = tuple(v - (1 if a == axis else 0) for a, v in enumerate(margins[key]))
                only = {k: (noise[k] if k == key else torch.zeros_like(noise[k])) for k in noise}
                got = step(**_perturbed(state, only, less))
                assert float((got[what][inside] - ref[what][inside]).abs().max()) > 0.0, (what, key, axis)


def test_schedule_of_a_whole_flow():
    """Backwards from the mask's cells the rectangles grow until they are the whole map; a frame-filling mask restricts nothing."""
    taps = {"convc1": (0, 0), "convc2": (1, 1), "convf1": (3, 3), "convf2": (1, 1), "convm": (1, 1), "gru0": (0, 2), "gru1": (2, 0),
            "fh1": (1, 1), "fh2": (1, 1), "mk1": (1, 1), "mk2": (0, 0)}
    hf, wf = 135, 240
    launches = flow_region.flow_launches(taps, 12)
    rects, need = flow_region.schedule(launches, flow_region.final_need((33, 60, 69, 120), hf, wf), hf, wf)
    area = {}
    for (it, tag, _), rr in zip(launches, rects):
        assert all(r is not None for r in rr)
        if tag == "convm":
            area[it] = rr[0][2] * rr[0][3] / (hf * wf)
    assert all(area[it] == 1.0 for it in range(7)) and area[7] < 1.0
    assert [round(area[it], 2) for it in (11, 10, 9)] == [0.34, 0.51, 0.70]
    assert flow_region.is_full(need["coords"], hf, wf) and flow_region.is_full(need["net0"], hf, wf)
    # every consumer's reads lie inside what its producer made: replay the schedule forwards
    made = {"coords": (0, 0, hf, wf), "flow": (0, 0, hf, wf), "net0": (0, 0, hf, wf)}
    for (it, tag, parts), rr in zip(launches, rects):
        for (name, reads, writes), r in zip(parts, rr):
            for buf, ry, rx in reads:
                want, have = flow_region.dilate(r, ry, rx, hf, wf), made[buf]
                assert flow_region.union(want, have) == have, (it, tag, name, buf)
            for w in writes:
                made[w] = r
    rects, _ = flow_region.schedule(launches, flow_region.final_need((0, 0, hf, wf), hf, wf), hf, wf)
    assert all(flow_region.is_full(r, hf, wf) for rr in rects for r in rr)
