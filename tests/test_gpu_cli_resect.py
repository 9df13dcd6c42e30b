"""`city2ba resect` on the GPU: the file it writes is, byte for byte, the file Python writes after BAProblem.resect_cameras
on the same input, and the counts it prints are that call's."""
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import _resectref as T
from test_gpu_schur_step import env  # noqa: F401  (env is the module fixture)
from test_gpu_resect import _load

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("opts", [{}, dict(min_points=9, min_gap=1e-3)], ids=["default", "9-points-gap-1e-3"])
def test_cli_resect_writes_what_python_writes(env, tmp_path, opts):
    import city2ba_amd as c2b
    src, out_cli, out_py = (str(tmp_path / n) for n in ("in.bbal", "out.bbal", "py.bbal"))
    ba = _load(T.dome_case(False, 1e-3))
    ba.write(src)
    ba.close()
    args = []
    if opts:
        args = ["--min-points", str(opts["min_points"]), "--min-gap", repr(opts["min_gap"])]
    run = subprocess.run([entry.build_cli(), "resect", src, out_cli] + args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)

    ba = c2b.BAProblem.from_file(src)
    before = ba.cameras_bal()
    ref = T.reference(ba.cameras(), ba.points(), ba.row_ptr, ba.pt_idx, ba.observations().reshape(-1, 2), bound=False,
                      **{k: v for k, v in opts.items()})
    assert len(T.cap_violations(ref)) == 0
    counts = ba.resect_cameras(**opts)
    moved = (ba.cameras_bal() != before).any(axis=1).sum()
    ba.write(out_py)
    ba.close()
    assert open(out_cli, "rb").read() == open(out_py, "rb").read()
    m = re.findall(r"(?m)^resected (\d+) cameras; kept: (\d+) too few observations, (\d+) degenerate, (\d+) behind a point, (\d+) constant$", run.stdout)
    assert m == [tuple(str(counts[k]) for k in T.STATUS)], run.stdout
    assert counts["resected"] > 40 and moved == counts["resected"]
    assert counts == T.counts_of(ref["status"])                  # the reference's counts at these options, on the file's own content
    if opts:                                                     # nine points and a wider gap keep cameras the defaults resect
        assert counts["resected"] < 63 and counts["too_few"] > 18
