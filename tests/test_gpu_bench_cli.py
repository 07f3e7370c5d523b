"""bench.py's command line on the GPU (C2, one pair, a few steps): `--steps` sets the number of timed steps, the result
line carries `ms_per_step`, `--dump-outputs DIR` writes the last timed registration's result as float32 / float64 .npy
files that are the same from run to run (seeded inputs), and a run without `--full` measures no CPU baseline."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _run(capsys, dump, steps):
    rc = bench.main(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--pairs", "1", "--dump-outputs", str(dump)])
    assert rc == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return line, {n[:-4]: np.load(dump / n) for n in sorted(os.listdir(dump))}


def test_plain_run_dumps_its_last_step(capsys, tmp_path):
    line, a = _run(capsys, tmp_path / "a", 3)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "scans/s" and line["higher_is_better"] is True and line["dtype"] == "f32 (f64 accumulate)"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] / 1000.0 - 1.0) < 1e-2  # value = steps / timed seconds
    assert line["cpu_baseline"] is None and "vs_cpu" not in line
    assert sorted(a) == ["final_tf", "result"]
    assert a["final_tf"].dtype == np.float32 and a["final_tf"].shape == (4, 4)
    assert a["result"].dtype == np.float64 and a["result"].shape == (7,)
    assert np.all(np.isfinite(a["final_tf"])) and np.array_equal(a["final_tf"][3], [0, 0, 0, 1])
    # nr_iterations, converged, trans_probability, score, n_passes, n_pairs, solver_fallbacks: the bench's fixed work
    assert a["result"][0] == 32 and a["result"][4] == 33 and a["result"][5] > 0
    # the same arguments give the same inputs, hence (one pair, deterministic kernels) the same outputs
    _, b = _run(capsys, tmp_path / "b", 2)
    assert np.array_equal(a["final_tf"], b["final_tf"]) and np.array_equal(a["result"], b["result"])
