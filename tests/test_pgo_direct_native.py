"""The pose graph's direct solve without a GPU: the Schur block of csrc/ndt_pgo_schur.h (the text k_pgo_schur runs) and
Woodbury's step on the host (tests/native/pgo_schur_check.cpp), and the solver surface of the C-ABI."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_schur_block_and_woodbury_step_on_the_host(tmp_path):
    """A seeded 12-node chain, three loops (one nested, one reversed), two position factors (one on node 0), d = 24: the
    block from the prefix table against B B^T formed densely, and the step against a dense solve of (I + B^T B) y = g.
    Both sides are the same f64 sums in different orders: 1e-12 relative to the largest entry."""
    exe = tmp_path / "pgo_schur_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "native", "pgo_schur_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    got = {ln.split()[0]: float(ln.split()[1]) for ln in out.stdout.splitlines()}
    assert set(got) == {"schur_block", "woodbury_step"}
    assert got["schur_block"] <= 1e-12 and got["woodbury_step"] <= 1e-12
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no host C compiler")
def test_solver_surface_of_the_abi(tmp_path):
    """The new constants, entry points and the stats struct exist, the struct matches its ctypes mirror, the layout version
    did not move, and a NULL handle is refused without a device."""
    from xchu_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    assert re.search(r"#define NDT_PGO_SOLVER_CG 0\b", hdr) and re.search(r"#define NDT_PGO_SOLVER_DIRECT 1\b", hdr)
    assert (_lib.PGO_SOLVER_CG, _lib.PGO_SOLVER_DIRECT) == (0, 1)
    lib = _lib.load()
    for name in ("ndt_pgo_set_solver", "ndt_pgo_get_solver", "ndt_pgo_solver_stats"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", hdr), name
    assert int(re.search(r"#define NDT_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6 == lib.ndt_abi_version()
    assert "ndt_pgo_set_solver" in hdr.split("#define NDT_HIP_ABI_VERSION")[0]       # the history records the addition
    assert lib.ndt_pgo_set_solver(None, 1) == _lib.NDT_EINVAL and lib.ndt_pgo_get_solver(None) == -1
    assert lib.ndt_pgo_solver_stats(None, None) == _lib.NDT_EINVAL
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "ndt_hip.h"', "int main(void) {",
           'printf("size %zu\\n", sizeof(ndt_pgo_solver_stats_t));']
    for f, _ in _lib.PgoSolverStats._fields_:
        src.append(f'printf("{f} %zu\\n", offsetof(ndt_pgo_solver_stats_t, {f}));')
    src.append("return NDT_PGO_SOLVER_DIRECT - 1; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.PgoSolverStats)
    for f, _ in _lib.PgoSolverStats._fields_:
        assert int(got[f]) == getattr(_lib.PgoSolverStats, f).offset, f
