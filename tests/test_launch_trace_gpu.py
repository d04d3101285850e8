"""The engine's launch sequence, call by call, against tests/golden/launch_traces.json (tests/launch_trace.py: the canonical form
of a call, the scenarios, the recorder).  The host code may be rearranged freely; the C calls, their arguments, their order and
the aliasing of their buffers may not move without the fixture's diff showing it."""
import json

import pytest

import launch_trace as LT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return json.loads(LT.FIXTURE.read_text())


def test_fixture_covers_every_scenario(recorded):
    assert sorted(recorded) == sorted(LT.SCENARIOS)


@pytest.mark.parametrize("name", list(LT.SCENARIOS))
def test_launches_match_the_recorded_trace(recorded, monkeypatch, name):
    want = recorded[name]
    got, crc = LT.run_scenario(name, monkeypatch)
    diff = LT.first_difference(want["calls"], got)
    if diff is not None:
        print(f"scenario {name}: first differing call is #{diff[0]} ({len(want['calls'])} recorded, {len(got)} made)\n"
              f"  recorded: {diff[1]}\n  this run: {diff[2]}")
    assert diff is None, f"{name}: call #{diff[0]}: recorded {diff[1]!r}, this run {diff[2]!r}"
    if want["out_crc"] is not None:             # (null: the recording commit's own two runs did not agree)
        assert crc == want["out_crc"], f"{name}: same launches, other outputs ({crc:08x}, recorded {want['out_crc']:08x})"
