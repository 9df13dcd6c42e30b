"""`city2ba refine --cameras` and `--alternate N` without a GPU: the help names the flags after the text it already had, every
bad value fails while the arguments are parsed, before a file is read or a device touched, and `refine` without the new flags
parses what it parsed."""
import os
import subprocess

import __graft_entry__ as entry


def _run(*args):
    return subprocess.run([entry.build_cli()] + list(args), capture_output=True, text=True, timeout=60)


def test_help_names_the_new_flags_after_the_old_ones():
    out = _run("refine", "--help")
    assert out.returncode == 0
    for flag in ("--cameras ", "--alternate <N>", "--rounds <N> [10]", "--lambda <L> [1e-4]", "--parameter-tol <T> [0]", "--device <N>"):
        assert flag in out.stdout, flag
    assert out.stdout.index("--alternate <N>") > out.stdout.index("--cameras ") > out.stdout.index("A point is written only when its cost fell.")
    top = _run("--help").stdout
    assert top.index("    refine ") > top.index("    rematch ") > top.index("    merge ")


def test_bad_values_fail_before_the_device(tmp_path):
    a, b = str(tmp_path / "a.bal"), str(tmp_path / "b.bal")                  # neither exists: a parsed command would fail on the read
    for args, message in ((("--alternate", "-1"), "Invalid value for '--alternate <alternate>'"), (("--alternate", "two"), "Invalid value for '--alternate <alternate>'"),
                          (("--alternate", "1000001"), "Invalid value for '--alternate <N>': expected an integer in 0 ... 1000000"),
                          (("--alternate",), "requires a value but none was supplied"),
                          (("--cameras", "--alternate", "2"), "The argument '--cameras' cannot be used with '--alternate <N>'"),
                          (("--cameras", "--rounds", "-1"), "Invalid value for '--rounds <rounds>'"),
                          (("--cameras", "--lambda", "0"), "Invalid value for '--lambda <L>': expected a number in 1e-20 ... 1e32"),
                          (("--alternate", "2", "--gradient-tol", "inf"), "Invalid value for '--gradient-tol <T>': expected a finite number >= 0"),
                          (("--points",), "--points")):
        r = _run("refine", a, b, *args)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    assert not os.path.exists(b)
    for args in (("--cameras",), ("--alternate", "3"), ("--cameras", "--rounds", "3", "--loss", "cauchy", "--loss-scale", "0.5"), ()):
        ok = _run("refine", a, b, *args)                                      # parsed: the read fails
        assert ok.returncode != 0 and "Invalid value" not in ok.stderr and "cannot be used" not in ok.stderr, (args, ok.stderr)
