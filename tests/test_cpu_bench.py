"""CPU: ``bench.py --gpus N`` started without a launcher starts N ranks itself (one process per
GPU under torch.distributed.run) from a parent that makes no GPU call — the driver's multi-GPU
scaling command depends on it (the N-GPU line used to time one rank)."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_spawns_n_ranks():
    env = dict(os.environ)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(v, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3",
                        "--selftest-spawn", "--no-cpu"], capture_output=True, text=True,
                       env=env, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert sorted(d["rank"] for d in lines) == [0, 1, 2]
    assert {d["world"] for d in lines} == {3}
    assert sorted(d["local_rank"] for d in lines) == [0, 1, 2]


def test_world_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
                        "--no-cpu"], capture_output=True, text=True, env=env, timeout=300,
                       cwd=ROOT)
    assert p.returncode != 0 and "WORLD_SIZE=1" in (p.stderr + p.stdout)


def test_torchrun_without_gpus_takes_launcher_world():
    """``torchrun --nproc-per-node 2 bench.py`` (no --gpus): the ranks take WORLD_SIZE from the
    launcher instead of refusing."""
    env = dict(os.environ)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(v, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port",
                        "29613", os.path.join(ROOT, "bench.py"), "--selftest-spawn", "--no-cpu"],
                       capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert sorted(d["rank"] for d in lines) == [0, 1]
    assert {d["world"] for d in lines} == {2}


def test_dump_samples_large_arrays_at_fixed_positions(tmp_path):
    n, limit = 1000, 64
    d = {"idx": torch.arange(10, dtype=torch.int32), "val": torch.arange(10.0),
         "out": torch.arange(float(n)), "counter": torch.arange(n, dtype=torch.int32)}
    bench.dump_outputs(str(tmp_path / "a"), d, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), d, limit=limit)
    a = {nm: np.load(tmp_path / "a" / f"{nm}.npy") for nm in ("idx", "val", "decoded", "counter")}
    assert a["idx"].shape == (10,) and a["decoded"].shape == (limit,)
    # the sample is the same positions for every array of that length, ascending, run to run
    np.testing.assert_array_equal(a["decoded"], a["counter"])
    assert np.all(np.diff(a["decoded"]) >= 0) and a["decoded"].max() < n
    np.testing.assert_array_equal(a["decoded"], np.load(tmp_path / "b" / "decoded.npy"))


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_a_long_plain_run_times_steps_once():
    """Regions per launch mode: 5..25 where both modes are timed at --steps; where only the
    chosen mode is, all regions together stay within max(--steps, 4000) steps."""
    assert bench.auto_repeats(20, True) == 25 and bench.auto_repeats(100000, True) == 5
    for steps in (201, 800, 1000, 2001, 4000, 4001, 10 ** 6):
        r = bench.auto_repeats(steps, False)
        assert r >= 1 and r * steps <= max(steps, 4000)
