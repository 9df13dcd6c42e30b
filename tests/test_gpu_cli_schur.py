"""`city2ba solve IN OUT --schur explicit` writes the file the Python route gives, byte for byte (BAProblem.from_file,
solve.levenberg_marquardt_device(schur="explicit") with the command's defaults, write), so its error is that route's."""
import subprocess

import pytest

from _problems import dome_problem

pytestmark = pytest.mark.gpu


def test_the_command_writes_what_the_python_route_writes(tmp_path):
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd as c2b
    from city2ba_amd import solve as S
    from city2ba_amd.baproblem import write_bal
    cli = entry.build_cli()
    P = dome_problem(dup=True)
    src, by_cli, by_py = str(tmp_path / "dome.bal"), str(tmp_path / "cli.bal"), str(tmp_path / "py.bal")
    write_bal(src, P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])
    r = subprocess.run([cli, "solve", src, by_cli, "--schur", "explicit", "--iterations", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ba = c2b.BAProblem.from_file(src)
    e0 = ba.total_reprojection_error(2.0)
    hist, summary = S.levenberg_marquardt_device(ba, 4, schur="explicit")
    assert ba.schur() == "explicit" and summary["final_cost"] < summary["initial_cost"]
    ba.write(by_py)
    e1 = ba.total_reprojection_error(2.0)
    ba.close()
    a, b = open(by_cli, "rb").read(), open(by_py, "rb").read()
    assert a == b and a != open(src, "rb").read()
    back = c2b.BAProblem.from_file(by_cli)
    assert back.total_reprojection_error(2.0) == pytest.approx(e1, rel=1e-9) and e1 < e0      # (the file holds 17 digits)
    back.close()
