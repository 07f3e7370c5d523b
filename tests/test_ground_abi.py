"""The ground surface of the C-ABI without a GPU: the two size-checked structs against their ctypes mirrors, the size
check itself, the defaults, and the layout version, which the surface does not move."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT


def test_ground_struct_layouts(tmp_path):
    from xchu_slam_amd import _lib
    structs = {"ndt_ground_params": _lib.GroundParams, "ndt_ground_result": _lib.GroundResult}
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "ndt_hip.h"', "int main(void) {"]
    for cname, py in structs.items():
        src.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            src.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
        assert py._fields_[0][0] == "struct_size" and getattr(py, "struct_size").offset == 0


def test_wrong_struct_size_is_refused():
    from xchu_slam_amd import _lib
    lib = _lib.load()
    p = _lib.GroundParams()
    for size in (0, ctypes.sizeof(_lib.GroundParams) - 4, ctypes.sizeof(_lib.GroundParams) + 8):
        p.struct_size = size
        p.normal_k = -7
        assert lib.ndt_ground_default_params(ctypes.byref(p)) == _lib.NDT_EINVAL
        assert p.normal_k == -7  # nothing was written
    assert lib.ndt_ground_default_params(None) == _lib.NDT_EINVAL
    p.struct_size = ctypes.sizeof(_lib.GroundParams)
    assert lib.ndt_ground_default_params(ctypes.byref(p)) == _lib.NDT_OK


def test_ground_defaults_are_filter_nodes():
    """filter_node.h:62-71, filter_node.cpp:36, 81, 151 and pcl::SampleConsensus's constructor."""
    from xchu_slam_amd import _lib
    from xchu_slam_amd.ground import ground_params
    import ground_restate as gr
    p = ground_params(_lib.load())
    for k, v in gr.DEFAULTS.items():
        assert getattr(p, k) == v, k
    assert abs(p.cloud_leaf - 0.2) < 1e-7 and p.struct_size == ctypes.sizeof(_lib.GroundParams)
    assert _lib.load().ndt_ground_batch() >= 1


def test_version_is_still_6_and_the_history_records_the_surface():
    from xchu_slam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    assert int(re.search(r"#define NDT_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6
    assert _lib.ABI_VERSION == 6 and _lib.load().ndt_abi_version() == 6
    assert "ground surface added at 6, size-checked" in hdr
