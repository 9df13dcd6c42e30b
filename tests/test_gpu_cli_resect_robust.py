"""`city2ba resect --max-error` on the GPU: the file it writes is, byte for byte, the file Python writes after
BAProblem.resect_cameras_robust with the same arguments on the same input, and the counts it prints are that call's."""
import re
import subprocess

import pytest

import __graft_entry__ as entry
import _resectrobustref as RR
from test_gpu_schur_step import env  # noqa: F401  (env is the module fixture)
from test_gpu_resect import _load

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("extra,kw", [(["--drop-outliers"], dict(drop_outliers=True)),
                                      (["--min-inliers", "8", "--max-hypotheses", "8", "--min-gap", "1e-3"], dict(min_inliers=8, max_hypotheses=8, min_gap=1e-3))],
                         ids=["drop-outliers", "flags"])
def test_cli_resect_max_error_writes_what_python_writes(env, tmp_path, extra, kw):
    import city2ba_amd as c2b
    src, out_cli, out_py = (str(tmp_path / n) for n in ("in.bbal", "out.bbal", "py.bbal"))
    ba = _load(RR.wrong_match_dome_cameras(False, 1e-3))
    ba.write(src)
    ba.close()
    run = subprocess.run([entry.build_cli(), "resect", src, out_cli, "--max-error", repr(RR.MAX_ERROR)] + extra, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)

    ba = c2b.BAProblem.from_file(src)
    n_obs = ba.num_observations()
    out = ba.resect_cameras_robust(RR.MAX_ERROR, **kw)
    assert ba.num_observations() == n_obs - out["removed"]
    ba.write(out_py)
    ba.close()
    assert open(out_cli, "rb").read() == open(out_py, "rb").read()
    m = re.findall(r"(?m)^resected (\d+) cameras; kept: (\d+) too few observations, (\d+) degenerate, (\d+) behind a point, (\d+) constant, "
                   r"(\d+) without consensus\n(\d+) outlier observations, (\d+) removed$", run.stdout)
    assert m == [tuple(str(out[k]) for k in RR.STATUS + ("outliers", "removed"))], run.stdout
    assert out["resected"] > 40 and out["outliers"] > 200
    assert out["removed"] == (out["outliers"] if kw.get("drop_outliers") else 0)
