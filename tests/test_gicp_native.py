"""The GICP control step's host run (tests/native/gicp_control_check.cpp: the NDT_HD text of csrc/ndt_gicp.h the device's
last workgroup runs, with a host evaluator) against tests/gicp_restate.py: the same trial points, statuses and
transformation over the first two outer iterations' pair sets of the small_pair scene."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gicp_restate as G
import icp_restate as R
from helpers import X_TOL, small_pair

HERE = os.path.dirname(os.path.abspath(__file__))


def _dump(path, pr, trans, prm):
    head = np.concatenate([[pr.m, prm["max_inner_iter"], prm["rot_eps"], prm["trans_eps"]],
                           np.asarray(pr.guess, np.float64).T.reshape(-1), np.asarray(trans, np.float64).T.reshape(-1)])
    body = np.concatenate([pr.p.astype(np.float64), pr.q.astype(np.float64), pr.gp.astype(np.float64), pr.M.reshape(pr.m, 9)], 1)
    np.concatenate([head, body.reshape(-1)]).astype(np.float64).tofile(path)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
@pytest.mark.parametrize("form", ["sensor_frame_guess", "map_frame_identity"])
def test_control_step_reproduces_restatement(tmp_path, form):
    exe = tmp_path / "gcc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "native", "gicp_control_check.cpp")], check=True)
    pair = small_pair(seed=3, n_source=4200)
    guess = pair.guess.astype(np.float32)
    if form == "sensor_frame_guess":
        src, g = pair.source[:1500], guess
    else:
        src, g = R.transform_f32(guess, pair.source[:1500]), None
    ref = G.gicp(src, pair.target, g, max_iter=2)
    assert len(ref["history"]) == 2
    prev = np.eye(4, dtype=np.float32)
    for it, h in enumerate(ref["history"]):
        path = tmp_path / f"pairs{it}.bin"
        _dump(path, h["pair_set"], prev, G.DEFAULTS)
        out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.splitlines()
        xs = np.array([[float.fromhex(t) for t in ln.split()[1:]] for ln in lines if ln.startswith("x ")])
        end = next(ln for ln in lines if ln.startswith("end ")).split()
        T = np.array([float.fromhex(t) for t in next(ln for ln in lines if ln.startswith("T")).split()[1:]]).reshape(4, 4).T
        trials = np.array(h["trials"])
        assert xs.shape == trials.shape, (xs.shape, trials.shape)
        worst = float(np.max(np.abs(xs - trials)))
        print(form, "iteration", it, "trials", len(xs), "worst |x - x_restatement|", worst, "status", G.MIN_NAMES[h["status"]])
        assert worst <= X_TOL
        assert (int(end[2]), int(end[4]), int(end[6])) == (h["status"], h["inner"], h["evals"])
        assert abs(float.fromhex(end[8]) - h["f"]) <= X_TOL * abs(h["f"])
        assert abs(float.fromhex(end[10]) - h["delta"]) <= 1e-9 * max(1.0, h["delta"])
        assert np.array_equal(T.astype(np.float32), h["T"])
        prev = h["T"]
