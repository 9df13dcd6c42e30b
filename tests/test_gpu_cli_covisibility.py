"""`city2ba covisibility IN [--min-shared K]` prints the reference's figures of a written dome, and `city2ba solve IN OUT
--window-around C [--hops N] [--min-shared K] [--max-cameras M] [--no-halo]` writes the file the Python calls give, byte for byte:
BAProblem.from_file, solve.solve_neighbourhood with the command's defaults, write."""
import subprocess

import pytest

import _covisref as CR
from _problems import dome_problem

pytestmark = pytest.mark.gpu


def _written_dome(tmp_path):
    from city2ba_amd.baproblem import write_bal
    P = dome_problem(dup=True)
    src = str(tmp_path / "dome.bal")
    write_bal(src, P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])
    return P, src


@pytest.mark.parametrize("min_shared", (1, 2, 5, 20))
def test_the_covisibility_line_is_the_references(tmp_path, min_shared):
    import __graft_entry__ as entry
    entry.build()
    cli = entry.build_cli()
    P, src = _written_dome(tmp_path)
    edges, max_degree, isolated = CR.figures(CR.graph(P["row_ptr"], P["pt_idx"], min_shared)[0])
    assert (edges, max_degree, isolated) == {1: (3160, 79, 1), 2: (1611, 72, 7), 5: (453, 62, 18), 20: (38, 29, 51)}[min_shared]
    r = subprocess.run([cli, "covisibility", src, "--min-shared", str(min_shared)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = "covisibility at %d shared points: 81 cameras, %d edges, maximum degree %d, %d isolated cameras" % (min_shared, edges, max_degree, isolated)
    assert r.stdout.strip().splitlines()[-1] == want, r.stdout


@pytest.mark.parametrize("halo", [True, False], ids=["halo", "nohalo"])
def test_the_command_writes_what_solve_neighbourhood_writes(tmp_path, halo):
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd as c2b
    from city2ba_amd import solve as S
    cli = entry.build_cli()
    P, src = _written_dome(tmp_path)
    by_cli, by_py = str(tmp_path / "cli.bal"), str(tmp_path / "py.bal")
    r = subprocess.run([cli, "solve", src, by_cli, "--window-around", "21,40", "--hops", "2", "--min-shared", "5", "--max-cameras", "30",
                        "--iterations", "4"] + ([] if halo else ["--no-halo"]), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ba = c2b.BAProblem.from_file(src)
    s = S.solve_neighbourhood(ba, [21, 40], hops=2, min_shared=5, max_cameras=30, halo=halo, iterations=4)
    assert len(s["seeds"]) == 30 and s["final_cost"] < s["initial_cost"]
    assert "neighbourhood of 2 cameras: 2 hops at 5 shared points: 30 cameras" in r.stdout
    assert "window: %d cameras, %d points, %d observations" % (s["cameras"], s["points"], s["observations"]) in r.stdout
    assert "written back: %d cameras, %d points" % (s["written"]["cameras"], s["written"]["points"]) in r.stdout
    ba.write(by_py)
    ba.close()
    a, b = open(by_cli, "rb").read(), open(by_py, "rb").read()
    assert a == b and a != open(src, "rb").read()


def test_option_conflicts_exit_non_zero_with_a_message(tmp_path):
    import __graft_entry__ as entry
    entry.build()
    cli = entry.build_cli()
    P, src = _written_dome(tmp_path)
    out = str(tmp_path / "out.bal")
    for args, message in ((("--window-around", "21", "--window", "0:10"), "cannot be used together"), (("--hops", "2"), "--hops needs --window-around"),
                          (("--window-around", "81"), "has 81 cameras, camera 81 was given"),
                          (("--window-around", "21,22,23", "--max-cameras", "2"), "Invalid value for '--max-cameras <M>'")):
        r = subprocess.run([cli, "solve", src, out] + list(args), capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
