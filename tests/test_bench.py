"""bench.py's multi-rank plumbing on the CPU (gloo, world size 2), through the real spawn path:
``python bench.py --gpus 2`` (no WORLD_SIZE) re-launches itself under torch.distributed.run with two
ranks, which count devices, run the (stand-in) clip forward, gather each step's depth to rank 0,
take the max over ranks and print one JSON line.  ``--dry-run`` swaps the HIP forward for a CPU
stand-in, so the numbers are not measurements; the GPU path is covered by the bench runs themselves."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.setdefault("OMP_NUM_THREADS", "2")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--dry-run", *args], capture_output=True,
                       text=True, timeout=300, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 prints exactly one line
    return json.loads(lines[0])


@pytest.mark.parametrize("gpus", [1, 2])
def test_bench_spawns_ranks_and_gathers(gpus):
    d = run_bench("--gpus", str(gpus), "--steps", "3", "--warmup", "1", "--frames", "4", "--size", "28", "28")
    assert d["config"]["ranks"] == gpus and d["n_gpus"] == gpus
    assert d["config"]["depth_gather_to_rank0"] == (gpus > 1)
    assert d["steps"] == 3 and d["unit"] == "frames/s" and d["scaling"] == "weak"
    assert abs(d["value"] - gpus * 3 * 4 / (d["ms_per_step"] * 3 / 1e3)) / d["value"] < 0.01


def test_bench_video_mode_two_ranks():
    d = run_bench("--gpus", "2", "--video", "--video-frames", "30", "--steps", "1", "--warmup", "0",
                  "--size", "28", "28")
    assert d["config"]["windows"] == 2 and d["scaling"] == "strong" and d["unit"] == "video frames/s"


def test_bench_dump_outputs_repeatable_and_full_flag(tmp_path):
    """--dump-outputs writes the last timed step's depth as float32 .npy, identical from run to run; a
    plain line carries null roofline / cpu_baseline, and --full is accepted."""
    import numpy as np
    common = ("--steps", "2", "--warmup", "1", "--frames", "4", "--size", "28", "28")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = run_bench(*common, "--dump-outputs", a)
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["roofline"] is None and d["cpu_baseline"] is None
    run_bench(*common, "--full", "--dump-outputs", b)
    da, db = np.load(os.path.join(a, "depth.npy")), np.load(os.path.join(b, "depth.npy"))
    assert da.dtype == np.float32 and da.shape == (1, 4, 28, 28) and np.isfinite(da).all() and da.any()
    assert np.array_equal(da, db)
    assert sorted(os.listdir(a)) == ["depth.npy"]


def test_plain_run_drops_the_extra_legs_and_full_keeps_them():
    """The parsed arguments of a plain run switch the roofline probe and the CPU baseline off whatever
    else is asked; with --full they stay as given (probe on, the whole-clip baseline by default)."""
    sys.path.insert(0, REPO)
    import bench
    base = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
    for extra in ([], ["--cpu-baseline-frames", "4"], ["--streams", "1"]):
        a = bench.parse(base + extra)
        assert a.no_probe is True and a.cpu_baseline_frames == 0 and not a.full
    a = bench.parse(base + ["--full"])
    assert a.full and a.no_probe is False and a.cpu_baseline_frames == 32
    a = bench.parse(base + ["--full", "--no-probe", "--cpu-baseline-frames", "4"])
    assert a.no_probe is True and a.cpu_baseline_frames == 4


@pytest.mark.gpu
def test_full_run_reports_roofline_and_cpu_baseline():
    """On the GPU (ViT-S 4 x 70 x 98, two steps): a --full line carries the fc1 probe's launches (12
    blocks x 2 single-stream forwards after the timed region) and the CPU-oracle baseline of the clip."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--encoder", "vits", "--frames", "4", "--size", "70", "98", "--full",
                        "--cpu-baseline-frames", "4"], capture_output=True, text=True, timeout=200, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    f = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert f["steps"] == 2 and f["ms_per_step"] > 0 and f["unit"] == "frames/s"
    assert f["roofline"]["launches"] == 24 and f["roofline"]["achieved"] > 0
    assert f["cpu_baseline"]["frames"] == 4 and f["cpu_baseline"]["value"] > 0


def test_dump_outputs_samples_past_the_budget(tmp_path, monkeypatch):
    """An array past its share of the budget is written as a fixed seeded sample: values, flat indices
    and the full shape, the same indices on every call, and the files stay within the budget."""
    import numpy as np
    sys.path.insert(0, REPO)
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 64 * 1024)
    big = np.arange(40 * 50 * 60, dtype=np.float64).reshape(40, 50, 60)  # 480 kB as float32
    small = np.ones((3, 5), dtype=np.float32)
    for sub in ("p", "q"):
        bench.dump_outputs(str(tmp_path / sub), {"big": big, "small": small})
    p = str(tmp_path / "p")
    assert sorted(os.listdir(p)) == ["big.npy", "big_index.npy", "big_shape.npy", "small.npy"]
    assert sum(os.path.getsize(os.path.join(p, f)) for f in os.listdir(p)) <= 64 * 1024
    v, idx = np.load(os.path.join(p, "big.npy")), np.load(os.path.join(p, "big_index.npy"))
    assert v.dtype == np.float32 and idx.dtype == np.int64 and len(v) == len(idx) > 1000
    assert np.array_equal(v, big.reshape(-1)[idx].astype(np.float32)) and np.all(np.diff(idx) > 0)
    assert np.load(os.path.join(p, "big_shape.npy")).tolist() == [40, 50, 60]
    assert np.array_equal(idx, np.load(str(tmp_path / "q" / "big_index.npy")))
    assert np.array_equal(np.load(os.path.join(p, "small.npy")), small)


def test_bench_rejects_mismatched_world():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--dry-run", "--gpus", "4"],
                       capture_output=True, text=True, timeout=120, env=env, cwd=REPO)
    assert p.returncode == 2 and "WORLD_SIZE" in p.stderr
