"""bench.py's N > 1 path end to end on the 1-GPU test box: `python bench.py --gpus 8` launches 8 ranks itself
(torch.distributed.run on 127.0.0.1); with fewer than 8 devices the ranks share device 0 and gather over gloo
(WOFT_SINGLE_DEVICE) -- launch line, rendezvous, per-rank sequences, barrier + max-over-ranks timing, the all_gather of the
tracks and the JSON contract are the 8-GPU run's, only the transport (RCCL over xGMI) differs."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _run(extra, timeout=1200):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--full", "--no-cpu-baseline", "--no-ladder", "--no-alt-precisions",
           "--no-alt-corr", *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.lstrip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]                 # ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_bench_eight_ranks_dry_run():
    d = _run(["--gpus", "8", "--steps", "2", "--warmup", "1", "--height", "256", "--width", "320"])
    assert d["n_gpus"] == 8 and d["steps"] == 2 and d["scaling"] == "weak" and d["config"]["sequences"] == 8
    assert d["tracks_gathered"] == [8, 2]                      # every rank's track reached rank 0
    assert len(d["per_rank"]) == 8 and [r["rank"] for r in d["per_rank"]] == list(range(8))
    assert all(r["ms_per_step"] > 0 and r["host_cores"] >= 1 for r in d["per_rank"])
    slowest = max(r["ms_per_step"] for r in d["per_rank"])
    assert d["ms_per_step"] >= slowest * 0.999                 # value = all ranks' frames / the slowest rank's time
    assert abs(d["value"] - 8 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    assert "roofline" in d and d["metric"].startswith("tracked frames/sec")


def test_bench_line_carries_ladder_and_lost_frames():
    """Small-size run of the --full bench line's extra passes: the like-for-like ladder, the lost-frame pass (forced every
    4th frame; the local flow runs in the second buffer set, so the frame after it costs what a normal frame costs) and the
    >= 200-step steady-state figure; the two-sequences-on-one-GPU side pass."""
    env = dict(os.environ)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--full", "--no-cpu-baseline", "--no-alt-precisions", "--no-alt-corr",
           "--steps", "8", "--warmup", "2", "--height", "384", "--width", "512"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.lstrip().startswith("{")][-1])
    lad = d["reference_work"]
    assert lad["bf16x3_full_weight_head"]["tracks_identical_to_timed_run"] is True
    assert lad["fp32_full_weight_head"]["correlation"] == "otf" and lad["fp32_full_weight_head"]["steps"] >= 20
    lf = d["lost_frame"]
    assert lf["lost_frames"] == lf["frames"] // lf["forced_every"] > 0
    assert lf["lost_frame_ms"] > lf["normal_frame_ms"] > 0 and lf["frame_after_lost_ms"] > 0
    run2 = lf["runs_of_two"]              # round 6: the second lost frame of a run takes its source features from the previous local flow
    assert run2["source_features_reused_on_second"] is True and 0 < run2["second_lost_frame_ms"] < run2["first_lost_frame_ms"]
    assert d["steady_state"]["steps"] == 200 and d["steady_state"]["frames_per_s"] > 0
    two = d["two_sequences_one_gpu"]            # round 6: two trackers, two streams, two host threads of one process
    assert two["sequences"] == 2 and two["errors"] is None and two["aggregate_frames_per_s"] > 0
    assert len(d["per_rank"]) == 1


def test_eight_ranks_1080p_host_launch_loops():
    """8-GPU readiness without the node: eight ranks at the METRIC's size (1080 x 1920, 12 iterations), NUMA
    binding on, sharing the one device -- so the GPU side is 8x slower than on eight GPUs, but each rank's HOST side (the
    Python launch loop: ~180 enqueues + one result read per frame) is what it will be there.  Its time per frame must stay
    below a quarter of a single GPU's frame time, or eight loops on two sockets become the limiter of the 8-GPU run."""
    one = _run(["--steps", "6", "--warmup", "3"])
    gpu_ms = one["ms_per_step"]
    assert one["per_rank"][0]["host_busy_ms_per_step"] <= 0.25 * gpu_ms, one["per_rank"]
    assert os.environ.get("WOFT_BIND", "1") != "0"              # (the launch threads are pinned as on the 8-GPU node)
    d = _run(["--gpus", "8", "--steps", "4", "--warmup", "2"], timeout=1800)
    assert d["n_gpus"] == 8 and d["tracks_gathered"] == [8, 4] and d["config"]["resolution"] == [1080, 1920]
    busy = [r["host_busy_ms_per_step"] for r in d["per_rank"]]
    print(f"single-rank GPU frame {gpu_ms:.2f} ms; host launch loop per frame, 8 ranks: {[round(b, 2) for b in busy]} ms")
    assert max(busy) <= 0.25 * gpu_ms, (busy, gpu_ms)


def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run (no --full): exactly --steps timed steps, the headline fields and none of the extra passes; --dump-outputs
    writes what the last timed track() call returned, and two runs with the same arguments write the same arrays."""
    dumps = []
    for k in range(2):
        d_out = tmp_path / f"run{k}"
        cmd = [sys.executable, str(ROOT / "bench.py"), "--steps", "5", "--warmup", "2", "--height", "256", "--width", "320",
               "--dump-outputs", str(d_out)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ))
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.lstrip().startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 5 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
        assert abs(d["value"] - 5 / (d["ms_per_step"] * 5e-3)) < 1e-6 * d["value"] and d["unit"] == "frames/s"
        assert d["metric"].startswith("tracked frames/sec") and d["dtype"]
        for extra in ("roofline", "alt_precisions", "alt_corr", "reference_work", "lost_frame", "cpu_baseline", "steady_state"):
            assert extra not in d, extra
        files = sorted(p.name for p in d_out.glob("*.npy"))
        assert "H_cur2init.npy" in files and "meta_lost.npy" in files, files
        arrays = {f: np.load(d_out / f) for f in files}
        assert arrays["H_cur2init.npy"].shape == (3, 3) and all(a.dtype == np.float64 for a in arrays.values())
        assert np.isfinite(arrays["H_cur2init.npy"]).all() and sum(a.nbytes for a in arrays.values()) <= 64 << 20
        dumps.append(arrays)
    assert sorted(dumps[0]) == sorted(dumps[1])
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f
