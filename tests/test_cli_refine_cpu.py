"""`city2ba refine` and `city2ba solve --inner-iterations` without a GPU: the help names the flags after the text it already
had, and every bad value fails while the arguments are parsed, before a file is read or a device touched."""
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([entry.build_cli()] + list(args), capture_output=True, text=True, timeout=60)


def test_help_names_the_new_flags():
    out = _run("refine", "--help")
    assert out.returncode == 0
    for flag in ("city2ba refine <FILE> <OUT>", "--rounds <N> [10]", "--lambda <L> [1e-4]", "--loss <squared|huber|cauchy|soft-l1> [squared]",
                 "--loss-scale <A> [1]", "--function-tol <T> [0]", "--gradient-tol <T> [0]", "--parameter-tol <T> [0]", "--device <N>"):
        assert flag in out.stdout, flag
    top = _run("--help").stdout
    assert top.index("    refine ") > top.index("    rematch ") > top.index("    merge ")          # after the text the help already had
    solve = _run("solve", "--help").stdout
    assert "--inner-iterations <N> [0]" in solve and solve.index("--inner-iterations") > solve.index("--preconditioner")


def test_bad_values_fail_before_the_device(tmp_path):
    a, b = str(tmp_path / "a.bal"), str(tmp_path / "b.bal")                  # neither exists: a parsed command would fail on the read
    tol = ": expected a finite number >= 0"
    for args, message in ((("--rounds", "-1"), "Invalid value for '--rounds <rounds>'"), (("--rounds", "ten"), "Invalid value for '--rounds <rounds>'"),
                          (("--rounds", "1000001"), "Invalid value for '--rounds <N>': expected an integer in 0 ... 1000000"),
                          (("--lambda", "0"), "Invalid value for '--lambda <L>': expected a number in 1e-20 ... 1e32"),
                          (("--lambda", "1e33"), "Invalid value for '--lambda <L>'"), (("--lambda", "nan"), "Invalid value for '--lambda <L>'"),
                          (("--loss", "l2"), "Invalid value for '--loss <loss>': expected squared, huber, cauchy or soft-l1"),
                          (("--loss", "cauchy", "--loss-scale", "0"), "Invalid value for '--loss-scale <A>': expected a finite number > 0"),
                          (("--loss-scale", "inf"), "Invalid value for '--loss-scale <A>'"),
                          (("--function-tol", "-1"), "Invalid value for '--function-tol <T>'" + tol),
                          (("--gradient-tol", "inf"), "Invalid value for '--gradient-tol <T>'" + tol),
                          (("--parameter-tol", "nan"), "Invalid value for '--parameter-tol <T>'" + tol),
                          (("--rounds",), "requires a value but none was supplied"), (("--min-angle", "1"), "--min-angle")):
        r = _run("refine", a, b, *args)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    r = _run("refine", a)
    assert r.returncode != 0 and "<FILE> <OUT>" in r.stderr
    for args, message in ((("--inner-iterations", "-1"), "Invalid value for '--inner-iterations <inner-iterations>'"),
                          (("--inner-iterations", "two"), "Invalid value for '--inner-iterations <inner-iterations>'"),
                          (("--inner-iterations", "1001"), "Invalid value for '--inner-iterations <N>': expected an integer in 0 ... 1000"),
                          (("--loss", "l2"), "Invalid value for '--loss <loss>': expected squared, huber, cauchy or soft-l1")):
        r = _run("solve", a, b, *args)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    assert not os.path.exists(b)
    ok = _run("refine", a, b, "--rounds", "3", "--loss", "cauchy", "--loss-scale", "0.5", "--function-tol", "1e-9")      # parsed: the read fails
    assert ok.returncode != 0 and "Invalid value" not in ok.stderr
