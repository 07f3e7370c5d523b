"""The profiling stamps' one description (csrc/ndt_stamps.h) against its Python reader: the 22 column names of
ndt_pass_phases, kPhaseNames, are the three name tuples of NormalDistributionsTransform.timings (xchu_slam_amd/ndt.py),
in order.  That the block table dbg_read_blk copies and the one the decoder indexes have one size is a static_assert of
host_prof.hip and ndt_stamps.h: the library's build checks it."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_names():
    text = open(os.path.join(ROOT, "xchu_slam_amd", "csrc", "ndt_stamps.h")).read()
    m = re.search(r"kPhaseNames\[[^\]]*\]\s*=\s*\{(.*?)\};", text, re.S)
    assert m, "kPhaseNames not found"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    return re.findall(r'"([^"]*)"', body)


def _python_names():
    tree = ast.parse(open(os.path.join(ROOT, "xchu_slam_amd", "ndt.py")).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "timings")
    tuples = [n for n in ast.walk(fn) if isinstance(n, ast.Tuple) and n.elts and
              all(isinstance(e, ast.Constant) and isinstance(e.value, str) for e in n.elts)]
    tuples.sort(key=lambda n: (n.lineno, n.col_offset))
    return [[e.value for e in t.elts] for t in tuples]


def test_phase_names_match_the_python_reader():
    header = _header_names()
    groups = _python_names()
    assert len(header) == 22 and len(set(header)) == 22, header
    assert [len(g) for g in groups] == [7, 5, 10], groups
    assert [n for g in groups for n in g] == header
