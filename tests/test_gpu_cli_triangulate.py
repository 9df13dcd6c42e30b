"""`city2ba triangulate` on the GPU: the file it writes is, byte for byte, the file Python writes after
BAProblem.triangulate_points on the same input, and the counts it prints are that call's."""
import re
import subprocess

import numpy as np

import pytest

import __graft_entry__ as entry
import _triangref as T
from test_gpu_schur_step import env  # noqa: F401  (env is the module fixture)
from test_gpu_triangulate import _load, _reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("deg", [None, 20.0], ids=["default", "20-degrees"])
def test_cli_triangulate_writes_what_python_writes(env, tmp_path, deg):
    import city2ba_amd as c2b
    src, out_cli, out_py = (str(tmp_path / n) for n in ("in.bbal", "out.bbal", "py.bbal"))
    ba = _load(T.dome_case(False, 1e-3))
    ba.write(src)
    ba.close()
    run = subprocess.run([entry.build_cli(), "triangulate", src, out_cli] + ([] if deg is None else ["--min-angle", repr(deg)]),
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)

    ba = c2b.BAProblem.from_file(src)
    before = ba.points()
    ref = _reference(ba, float(np.deg2rad(1.0 if deg is None else deg)), bound=False)
    narrow = T.counts_of(_reference(ba, bound=False)["status"])                 # at the default of one degree
    assert len(T.cap_violations(ref)) == 0
    counts = ba.triangulate_points() if deg is None else ba.triangulate_points(min_angle_deg=deg)
    moved = (ba.points() != before).any(axis=1).sum()
    ba.write(out_py)
    ba.close()
    assert open(out_cli, "rb").read() == open(out_py, "rb").read()
    m = re.findall(r"(?m)^triangulated (\d+) points; kept: (\d+) too few observations, (\d+) degenerate, (\d+) behind a camera, (\d+) constant$", run.stdout)
    assert m == [tuple(str(counts[k]) for k in T.STATUS)], run.stdout
    assert counts["triangulated"] > 100 and moved == counts["triangulated"]
    assert counts == T.counts_of(ref["status"])              # the reference's counts at this angle, on the file's own content
    if deg is not None:                                      # a wider threshold rejects points the default accepts, by the reference's count
        assert counts["degenerate"] > narrow["degenerate"] and counts["triangulated"] < narrow["triangulated"]
