"""`city2ba solve` without a device: its help lists every flag, and argument errors come from the parser, in the wording
the other subcommands use, before anything touches a GPU."""
import subprocess

import __graft_entry__ as entry

FLAGS = ("--iterations", "--lambda", "--pcg-iterations", "--pcg-tol", "--function-tol", "--gradient-tol", "--parameter-tol",
         "--loss", "--loss-scale", "--preconditioner", "--fix-intrinsics", "--fix-first-camera")


def _run(*args):
    return subprocess.run([entry.build_cli()] + list(args), capture_output=True, text=True, timeout=60)


def test_help_lists_solve_and_every_flag():
    top = _run("--help")
    assert top.returncode == 0 and "solve" in top.stdout
    out = _run("solve", "--help")
    assert out.returncode == 0 and "city2ba solve <FILE> <OUT>" in out.stdout
    for flag in FLAGS:
        assert flag in out.stdout, flag
    for value in ("squared", "huber", "cauchy", "soft-l1", "block-jacobi", "schur-jacobi"):
        assert value in out.stdout, value


def test_argument_errors_need_no_device(tmp_path):
    a, b = str(tmp_path / "a.bal"), str(tmp_path / "b.bal")
    for args, message in ((("solve", a), "The following required arguments were not provided:\n    <FILE> <OUT>"),
                          (("solve", a, b, "--loss", "tukey"), "Invalid value for '--loss <loss>'"),
                          (("solve", a, b, "--iterations", "x"), "Invalid value for '--iterations <iterations>': invalid digit found in string"),
                          (("solve", a, b, "--lambda", "small"), "Invalid value for '--lambda <lambda>': invalid float literal"),
                          (("solve", a, b, "--preconditioner", "ssor"), "Invalid value for '--preconditioner <preconditioner>'"),
                          (("solve", a, b, "--trust-region"), "Found argument '--trust-region' which wasn't expected"),
                          (("solve", a, b, "--loss"), "The argument '--loss <loss>' requires a value but none was supplied")):
        out = _run(*args)
        assert out.returncode == 1 and out.stderr.startswith("Error: " + message), (args, out.returncode, out.stderr)
        assert "HIP" not in out.stderr and "device" not in out.stderr, out.stderr
