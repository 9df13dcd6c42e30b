"""`city2ba rematch` on the GPU: the file it writes is, byte for byte, the file Python writes after
BAProblem.rematch_observations with the same arguments on the same input, and the numbers it prints are that call's."""
import re
import subprocess

import pytest

import __graft_entry__ as entry
import _rematchref as R
from test_gpu_schur_step import env  # noqa: F401  (env is the module fixture)
from test_gpu_triangulate import _load

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ext,min_fits", [("bbal", None), ("bal", 0)], ids=["default-bbal", "min-fits-0-bal"])
def test_cli_rematch_writes_what_python_writes(env, tmp_path, ext, min_fits):
    import city2ba_amd as c2b
    src, out_cli, out_py = (str(tmp_path / n) for n in ("in." + ext, "out." + ext, "py." + ext))
    P = R.wrong_label_dome(False, 1e-3)
    ba = _load(P)
    ba.write(src)
    ba.close()
    extra = [] if min_fits is None else ["--min-fits", str(min_fits)]
    run = subprocess.run([entry.build_cli(), "rematch", src, out_cli, "--radius", repr(P["radius"]), "--max-error", repr(R.MAX_ERROR)] + extra,
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)

    ba = c2b.BAProblem.from_file(src)
    n_pts, n_obs = ba.num_points(), ba.num_observations()
    out = ba.rematch_observations(P["radius"], R.MAX_ERROR, **({} if min_fits is None else dict(min_fits=min_fits)))
    assert ba.num_points() == n_pts and ba.num_observations() == n_obs - out["removed"]        # nothing is culled
    ba.write(out_py)
    ba.close()
    assert open(out_cli, "rb").read() == open(out_py, "rb").read()
    assert open(out_cli, "rb").read() != open(src, "rb").read()
    m = re.findall(r"(?m)^reassigned (\d+) observations and removed (\d+) of (\d+); nothing is culled$", run.stdout)
    assert m == [(str(out["reassigned"]), str(out["removed"]), str(n_obs))], run.stdout
    assert out["reassigned"] > 300 and (out["skipped"] == 0) == (min_fits == 0)
