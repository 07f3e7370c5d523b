"""Host check of the pass kernels' in-wave reduce-scatter (csrc/ndt_rstree.h, tests/native/reduce_tree_check.cpp).

rs22_reduce (the 22 split sums in 11 + 6 + 3 + 2 + 1 = 23 exchanges) is run on emulated 64-lane waves and compared with an
emulation of the schedule it replaced (32 slots, rs_step<16> .. rs_step<1>): every value's wave total in both half-waves
bit for bit (NaN as NaN), on random doubles over the full exponent range, sums of like magnitude, +0.0 / -0.0 in every
position, infinities, NaNs and subnormals.  The program itself fails unless both half-waves and all 22 values were
compared and every value is reported by exactly one lane.  Built and run a second time with the host sanitizers."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_reduce_tree_bit_exact(tmp_path):
    src = os.path.join(HERE, "native", "reduce_tree_check.cpp")
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / ("rtc_" + tag)
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", str(exe), src], check=True)
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, tag + "\n" + out.stdout + out.stderr
        assert "mismatched: 0" in out.stdout and "map errors: 0" in out.stdout and "unseen (half, value): 0" in out.stdout
