"""`city2ba merge` on the GPU: the file it writes is, byte for byte, the file Python writes after BAProblem.merge_points with
the same arguments on the same input, and the number it prints is that call's."""
import re
import subprocess

import pytest

import __graft_entry__ as entry
import _mergeref as M
from test_gpu_schur_step import env  # noqa: F401  (env is the module fixture)
from test_gpu_triangulate import _load

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ext,max_error,rounds", [("bbal", 1e-4, 1), ("bal", 1e-2, 3)], ids=["recovery-bbal", "false-merges-bal"])
def test_cli_merge_writes_what_python_writes(env, tmp_path, ext, max_error, rounds):
    import city2ba_amd as c2b
    src, out_cli, out_py = (str(tmp_path / n) for n in ("in." + ext, "out." + ext, "py." + ext))
    S = M.split_dome()
    ba = _load(S["P"])
    ba.write(src)
    ba.close()
    run = subprocess.run([entry.build_cli(), "merge", src, out_cli, "--radius", "0.5", "--max-error", repr(max_error), "--rounds", str(rounds)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)

    ba = c2b.BAProblem.from_file(src)
    n_pts, n_obs = ba.num_points(), ba.num_observations()
    out = ba.merge_points(0.5, max_error, rounds=rounds)
    assert ba.num_points() == n_pts and ba.num_observations() == n_obs        # nothing is culled
    ba.write(out_py)
    ba.close()
    assert open(out_cli, "rb").read() == open(out_py, "rb").read()
    assert open(out_cli, "rb").read() != open(src, "rb").read()
    m = re.findall(r"(?m)^merged (\d+) points in (\d+) rounds; they stay in the file as unobserved points$", run.stdout)
    assert m == [(str(out["merged"]), str(out["rounds"]))], run.stdout
    assert out["merged"] >= len(S["both"]) and (out["merged"] > len(S["both"])) == (max_error > 1e-3)
