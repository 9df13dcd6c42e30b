"""`city2ba solve --linear-solver pcg|cholesky` without a GPU: the help and the file's header name the flag, `--schur` keeps its
usage line, and a bad, empty or missing value is refused with the option's usage line before a device is touched."""
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_names_the_flag():
    cli = entry.build_cli()
    out = subprocess.run([cli, "solve", "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--linear-solver <pcg|cholesky> [pcg]" in out.stdout
    assert "--schur <implicit|explicit> [implicit]" in out.stdout         # a new flag, not a third value of the old one
    head = open(os.path.join(ROOT, "city2ba_amd", "cli", "main.cpp")).read().split("#include", 1)[0]
    assert "--linear-solver pcg|cholesky" in head and "--schur implicit|explicit" in head


def test_a_bad_value_is_refused_before_the_device(tmp_path):
    cli = entry.build_cli()
    src, out = tmp_path / "in.bal", str(tmp_path / "out.bal")
    src.write_text("5 7 0\n")                                # the counts alone: a parsed command would fail on the read
    usage = "Invalid value for '--linear-solver <pcg|cholesky>'"
    for args, message in ((("--linear-solver", "dense"), usage), (("--linear-solver", "Cholesky"), usage), (("--linear-solver", "1"), usage),
                          (("--linear-solver", ""), usage), (("--linear-solver",), "requires a value but none was supplied"),
                          (("--linear-solver", "cholesky", "--schur", "dense"), "Invalid value for '--schur <implicit|explicit>'")):
        r = subprocess.run([cli, "solve", str(src), out] + list(args), capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    assert not os.path.exists(out)
