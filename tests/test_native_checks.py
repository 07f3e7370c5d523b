"""Host checks of device-side restatements that have a scalar twin (compiled with g++ -ffp-contract=off, run here).

* angle_table_entry (one lane per entry of computeAngleDerivatives' tables, ndt_omp_impl.hpp:286-398) vs
  angle_table_row: bit-exact on random angles (tests/native/angle_table_check.cpp).
* the derivative passes' launch geometry and the two-level hand-off's grouping (csrc/ndt_geom.h, ndt_types.h), swept over
  CU counts, searches, pass options and source sizes around every threshold (tests/native/pass_geom_check.cpp).
* the host steps every unit shares (csrc/ndt_geom.h): the strided-cloud packer, the xyzi layout rule and grid_for, also
  under the host sanitizers (tests/native/cloud_pack_check.cpp).
* the profiling stamps' decoder (csrc/ndt_stamps.h) on synthetic stamp tables, also under the host sanitizers
  (tests/native/stamp_decode_check.cpp).
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_angle_table_entries_bit_exact(tmp_path):
    exe = tmp_path / "atc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "native", "angle_table_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatched: 0" in out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_packed_pair_math_bit_exact(tmp_path):
    """pair_pk (the derivative pass's pair arithmetic as packed f32 pairs, ndt_pair.h) == pair_f32 (one f32 operation per
    reference operation, ndt_omp_impl.hpp:491-548) on 400 k random pairs, with and without the Hessian; and the predicated
    form the pass kernels call, pair_pk_terms<true>: equal to pair_f32 with valid = true, every sum untouched bit for bit
    with valid = false (the program itself fails unless >= 1 % of the pairs are rejected and >= 50 % accepted)."""
    exe = tmp_path / "ppc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "native", "pair_pk_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatched: 0" in out.stdout
    assert "predicated differ: 0" in out.stdout
    assert "masked changed: 0" in out.stdout

def _quadmath_ok(tmp_path) -> bool:
    src = tmp_path / "q.cpp"
    src.write_text("#include <quadmath.h>\nint main(){ return (int)expq((__float128)0); }\n")
    return subprocess.run(["g++", str(src), "-lquadmath", "-o", str(tmp_path / "q")], capture_output=True).returncode == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_libm_restatements_correctly_rounded(tmp_path):
    """exp_dr == RN_f32(RN_f64(e^x)) (updateDerivatives' (float)exp((double)x) with glibc 2.23's correctly rounded exp,
    libndt_omp.so 0x424a4-0x424bc) and sinf_dr / cosf_dr == the correctly rounded f32 sin / cos (the model of the
    binary's sincosf), against libquadmath wherever this host's double libm cannot decide: every 61st f32 bit pattern plus
    every 7th pattern of [-2, 0] (exp) and [-0.1, 0.1] (sin / cos).  Also asserts that the oracle's own expressions
    ((float)std::exp((double)x), (float)std::sin((double)x)) give the same values.  Exhaustive run (stride 1): see
    DESIGN.md section 2."""
    if not _quadmath_ok(tmp_path):
        pytest.skip("libquadmath not available")
    exe = tmp_path / "libm"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fopenmp", "-o", str(exe),
                    os.path.join(HERE, "native", "libm_check.cpp"), "-lquadmath"], check=True)
    out = subprocess.run([str(exe), "61"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatched: 0" in out.stdout
    for line in out.stdout.splitlines():
        if "host-libm-rounded differs" in line:
            assert "host-libm-rounded differs 0 " in line, line


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_pair_orders_match_binary_sse(tmp_path):
    """pair_f32 / pair_pk (the device's per-pair f32 arithmetic) and mat3_mul_f (convertTransform's rotation products)
    against a transcription of the shipped libndt_omp.so's instruction sequences into SSE intrinsics (updateDerivatives
    0x422a0 with its Eigen product callees, computePointDerivatives 0x4b650, Transform::rotate 0x3da70; read as text,
    never run): every accumulated value equal on 300 k random pairs (tests/native/sse_order_check.cpp)."""
    exe = tmp_path / "sse"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-msse2", "-o", str(exe),
                    os.path.join(HERE, "native", "sse_order_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatched: 0" in out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_pass_geometry_sweep(tmp_path):
    """The launch geometry host_align.hip launches through (ndt_geom.h), for 1 / 8 / 104 / 256 / 304 CUs, DIRECT7 /
    DIRECT26 / DIRECT1, points_per_thread 1 / 2 / 3, both tails and every source size within 2 of a threshold (4096,
    768 per CU, 262 144, 393 216, 1 048 576, the powers of two to 2^23) plus a stride: the size bucket is >= the scan,
    monotone and a whole number of its steps; every tile's points have a thread slot (ppb <= block x points per thread);
    the workgroups' tiles cover the bucket and one-tile kernels in one tile; two points per thread only while every
    cloud index fits 22 bits.  For every grid of 1025..32768 workgroups the two-level hand-off's group size is even (a
    group closer loads its columns as 16-byte pairs from partials + g * G), there are at most kMaxGroups groups, the
    last one is not empty and the group partials fit the allocation.  The geometries tests/test_gpu_pass_geometry.py
    names are pinned for 256 CUs."""
    exe = tmp_path / "pgc"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(HERE, "native", "pass_geom_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatched: 0" in out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_cloud_pack_and_grid_for(tmp_path):
    """The host steps every unit shares (csrc/ndt_geom.h), tests/native/cloud_pack_check.cpp: pack_cloud4 equals the
    literal strided loop for n = 0, 1, 5 and 1000 records of stride 12 (w = 1), 16 (intensity at float 3), 32 (at 4) and
    32 (at 7, the record's last float); xyzi_layout_ok rejects (2,32), (3,12), (8,32) and (4,16) and accepts (3,16),
    (4,32) and (7,32); grid_for at n = 0, 1, per, per + 1, cap * per and cap * per + 1.  Built and run a second time
    with -fsanitize=address,undefined (a stand-alone host program: the record buffers end with their last record)."""
    src = os.path.join(HERE, "native", "cloud_pack_check.cpp")
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / ("cpc_" + tag)
        subprocess.run(["g++", "-std=c++17", *flags, "-o", str(exe), src], check=True)
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, tag + "\n" + out.stdout + out.stderr
        assert "mismatched: 0" in out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_stamp_decoder(tmp_path):
    """accumulate_pass_stats (csrc/ndt_stamps.h: what ndt_last_timings / ndt_pass_phases report) on synthetic tables of at
    most 4 passes x 4 workgroups whose phases each last their own number of ticks, tests/native/stamp_decode_check.cpp:
    the seven product phases, the time and the 16 N + 36 pairs bytes of one pass; rows never stamped or ending before
    they start; a leading-tail row (timed, no phases); workgroup means with a workgroup past the scan's points and a
    pass dropped for a row out of order; the last-workgroup tail's eight phases and the speculative-solve pair, with one
    stamp out of order; the leading-tail kernel's tail from pass k's prologue row and pass k - 1's tail row (none for
    k = 0); a second round accumulating into the first; passes past the table and more workgroups than rows.  Built and
    run a second time with -fsanitize=address,undefined (a stand-alone host program: the tables are exactly as large as
    their shape says)."""
    src = os.path.join(HERE, "native", "stamp_decode_check.cpp")
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / ("sdc_" + tag)
        subprocess.run(["g++", "-std=c++17", *flags, "-o", str(exe), src], check=True)
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, tag + "\n" + out.stdout + out.stderr
        assert "mismatched: 0" in out.stdout
