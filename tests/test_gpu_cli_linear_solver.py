"""`city2ba solve IN OUT --linear-solver cholesky` on the small grid writes the file the Python route gives, byte for byte
(BAProblem.from_file, solve.levenberg_marquardt_device(linear_solver="cholesky") with the command's defaults, write), so its error is
that loop's; and no row of the loop ran a PCG iteration."""
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_the_command_writes_what_the_python_route_writes(tmp_path):
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd as c2b
    from city2ba_amd import solve as S
    from test_gpu_schur_step import _make
    cli = entry.build_cli()
    src, by_cli, by_py = str(tmp_path / "grid.bal"), str(tmp_path / "cli.bal"), str(tmp_path / "py.bal")
    g, _ = _make("small grid culled")
    g.write(src)
    g.close()
    r = subprocess.run([cli, "solve", src, by_cli, "--linear-solver", "cholesky", "--iterations", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ba = c2b.BAProblem.from_file(src)
    e0 = ba.total_reprojection_error(2.0)
    hist, summary = S.levenberg_marquardt_device(ba, 4, linear_solver="cholesky")
    assert ba.linear_solver() == "cholesky" and ba.schur() == "implicit" and summary["final_cost"] < summary["initial_cost"]
    assert [h["pcg_iterations"] for h in hist] == [0] * len(hist) and all(h["status"] == 0 for h in hist)
    ba.write(by_py)
    e1 = ba.total_reprojection_error(2.0)
    ba.close()
    a, b = open(by_cli, "rb").read(), open(by_py, "rb").read()
    assert a == b and a != open(src, "rb").read()
    back = c2b.BAProblem.from_file(by_cli)
    assert back.total_reprojection_error(2.0) == pytest.approx(e1, rel=1e-9) and e1 < e0      # (the file holds 17 digits)
    back.close()
