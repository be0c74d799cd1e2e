"""GPU: a ``bench.py`` run without ``--full`` times the headline only and prints only its line, and
``--dump-outputs`` writes what the last timed step computed — checked against the reference's op
sequence (oracle/ref_ops.py) on the same seeded inputs, so two builds' dumps are comparable."""
import json
import sys

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "stages", "cpu_baseline", "secondary", "gossip_round", "shard")


def test_plain_run_prints_the_headline_and_dumps_the_last_step(dev, tmp_path, monkeypatch, capsys):
    from oracle import ref_ops
    n, alpha, steps, warmup = 1_000_003, 0.01, 11, 2
    out = tmp_path / "dump"
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup",
                                      str(warmup), "--n", str(n), "--rotate", "3",
                                      "--dump-outputs", str(out)])
    bench.main()
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    # value is 4N bytes per step time in GiB/s (ms_per_step is rounded to 5 decimals)
    assert line["value"] == pytest.approx(4 * n / (line["ms_per_step"] * 1e-3) / 2 ** 30, rel=1e-2)
    assert not line["sampled_path_fell_back"]
    assert not [k for k in FULL_ONLY if k in line]

    # the same inputs (seed 1234 + rank, states generated in order), the reference's ops on them:
    # the last step is state L's, decoding state L - 1's payload (one-node mode runs last)
    R = line["config"]["rotated_states"]
    L = (steps - 1) % R
    g = torch.Generator(device=dev).manual_seed(1234)
    states = []
    for _ in range(R):
        x = torch.randn(n, device=dev, generator=g)
        x0 = x - 0.01 * torch.randn(n, device=dev, generator=g)
        states.append((x.cpu(), x0.cpu()))
    counter = torch.zeros(n, dtype=torch.int32)
    idx, val = ref_ops.encode(*states[L], alpha, counter)
    pidx, pval = ref_ops.encode(*states[(L - 1) % R], alpha, torch.zeros(n, dtype=torch.int32))
    decoded = ref_ops.decode(states[L][0], pidx, pval).numpy()

    got = {nm: np.load(out / f"{nm}.npy") for nm in ("idx", "val", "decoded", "counter")}
    assert got["idx"].dtype == np.float64 and got["val"].dtype == np.float32
    assert got["decoded"].dtype == np.float32 and got["counter"].dtype == np.float32
    np.testing.assert_array_equal(got["idx"], idx.astype(np.float64))
    np.testing.assert_array_equal(got["val"].view(np.uint32), val.view(np.uint32))
    np.testing.assert_array_equal(got["decoded"].view(np.uint32), decoded.view(np.uint32))
    # the model does not change between steps: every encode of the state shares the same k
    # entries, so its counter is (number of encodes) x the reference's one-encode counter
    c = counter.numpy().astype(np.float32)
    times = got["counter"].max()
    assert times >= 1 and times == int(times)
    np.testing.assert_array_equal(got["counter"], times * c)
