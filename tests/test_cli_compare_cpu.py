"""`city2ba compare EST REF` without a GPU: the help names the flags, the usage comment and the subcommand list name it, and every
malformed argument is refused before a device is created or a file is opened."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as entry
    entry.build_hip()
    return entry.build_cli()


def run(cli, *args):
    return subprocess.run([cli] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_help_names_the_flags_and_the_subcommand(cli):
    r = run(cli, "--help")
    assert r.returncode == 0 and "compare" in r.stdout
    r = run(cli, "compare", "--help")
    assert r.returncode == 0, r.stderr
    for flag in ("--on", "--no-scale", "--max-dist", "--rounds", "--apply", "--device"):
        assert flag in r.stdout, flag
    assert "consensus" in r.stdout and "too_few" in r.stdout       # what trimming is not, and how an emptied set shows
    src = open(os.path.join(ROOT, "city2ba_amd", "cli", "main.cpp")).read()
    assert "city2ba compare EST REF [--on cameras|points|both] [--no-scale] [--max-dist D [--rounds N]] [--apply OUT]" in src


def test_malformed_arguments_are_refused_before_a_device_or_a_file_is_touched(cli, tmp_path):
    est, ref, out = tmp_path / "missing_est.bbal", tmp_path / "missing_ref.bbal", tmp_path / "o.bbal"
    cases = ((("compare",), "required arguments"), (("compare", est), "required arguments"), (("compare", est, ref, out), "required arguments"),
             (("compare", est, ref, "--on", "everything"), "--on <KIND>"), (("compare", est, ref, "--on"), "requires a value"),
             (("compare", est, ref, "--max-dist", "0"), "--max-dist <D>"), (("compare", est, ref, "--max-dist", "-2"), "--max-dist <D>"),
             (("compare", est, ref, "--max-dist", "inf"), "--max-dist <D>"), (("compare", est, ref, "--max-dist", "x"), "invalid float literal"),
             (("compare", est, ref, "--max-dist", "1", "--rounds", "0"), "--rounds <N>"), (("compare", est, ref, "--rounds", "3"), "--rounds needs --max-dist"),
             (("compare", est, ref, "--max-dist", "1", "--rounds", "x"), "invalid digit"), (("compare", est, ref, "--bogus", "1"), "wasn't expected"),
             (("compare", est, ref, "--no-scale", "--apply"), "requires a value"))
    for args, word in cases:
        r = run(cli, *args)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)
        assert "HIP" not in r.stderr and "Could not open" not in r.stderr, (args, r.stderr)      # refused before either
        assert r.stdout == "" and not out.exists()
