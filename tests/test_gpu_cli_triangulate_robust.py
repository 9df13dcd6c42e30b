"""`city2ba triangulate --max-error` on the GPU: the file it writes is, byte for byte, the file Python writes after
BAProblem.triangulate_points_robust with the same arguments on the same input, and the counts it prints are that call's."""
import re
import subprocess

import pytest

import __graft_entry__ as entry
import _triangrobustref as RR
from test_gpu_schur_step import env  # noqa: F401  (env is the module fixture)
from test_gpu_triangulate import _load

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("extra,kw", [(["--drop-outliers"], dict(drop_outliers=True)),
                                      (["--min-inliers", "4", "--max-hypotheses", "8", "--min-angle", "2"], dict(min_inliers=4, max_hypotheses=8, min_angle_deg=2.0))],
                         ids=["drop-outliers", "flags"])
def test_cli_triangulate_max_error_writes_what_python_writes(env, tmp_path, extra, kw):
    import city2ba_amd as c2b
    src, out_cli, out_py = (str(tmp_path / n) for n in ("in.bbal", "out.bbal", "py.bbal"))
    ba = _load(RR.wrong_match_dome(False, 1e-3))
    ba.write(src)
    ba.close()
    run = subprocess.run([entry.build_cli(), "triangulate", src, out_cli, "--max-error", repr(RR.MAX_ERROR)] + extra, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)

    ba = c2b.BAProblem.from_file(src)
    n_obs = ba.num_observations()
    out = ba.triangulate_points_robust(RR.MAX_ERROR, **kw)
    assert ba.num_observations() == n_obs - out["removed"]
    ba.write(out_py)
    ba.close()
    assert open(out_cli, "rb").read() == open(out_py, "rb").read()
    m = re.findall(r"(?m)^triangulated (\d+) points; kept: (\d+) too few observations, (\d+) degenerate, (\d+) behind a camera, (\d+) constant, "
                   r"(\d+) without consensus\n(\d+) outlier observations, (\d+) removed$", run.stdout)
    assert m == [tuple(str(out[k]) for k in RR.STATUS + ("outliers", "removed"))], run.stdout
    assert out["triangulated"] > 200 and out["outliers"] > 200
    assert out["removed"] == (out["outliers"] if kw.get("drop_outliers") else 0)
