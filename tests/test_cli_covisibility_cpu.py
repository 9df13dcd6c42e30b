"""`city2ba solve --window-around C[,C...] [--hops N] [--min-shared K] [--max-cameras M]` and `city2ba covisibility` without a
GPU: the help names the flags, and every conflict and bad value is refused with a message before a device is touched."""
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_names_the_flags_and_the_subcommand():
    cli = entry.build_cli()
    out = subprocess.run([cli, "solve", "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    for text in ("--window-around <C[,C...]>", "--hops <N> [1]", "--min-shared <K> [1]", "--max-cameras <M>", "not with --window"):
        assert text in out.stdout, text
    out = subprocess.run([cli, "covisibility", "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--min-shared <K> [1]" in out.stdout
    assert "covisibility" in subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    head = open(os.path.join(ROOT, "city2ba_amd", "cli", "main.cpp")).read().split("#include", 1)[0]
    assert "[--window-around C[,C...] [--hops N] [--min-shared K] [--max-cameras M] [--no-halo]]" in head and "city2ba covisibility IN" in head


def test_conflicts_and_bad_values_are_refused_before_the_device(tmp_path):
    cli = entry.build_cli()
    src, out = tmp_path / "in.bal", str(tmp_path / "out.bal")
    src.write_text("5 7 0\n")                                # the counts alone: a parsed command would fail on the read
    bad = "Invalid value for '--window-around <C[,C...]>'"
    for args, message in ((("--window-around", "1", "--window", "0:2"), "cannot be used together"),
                          (("--window-around", ""), bad), (("--window-around", "1,"), bad), (("--window-around", ",1"), bad),
                          (("--window-around", "1,,2"), bad), (("--window-around", "a"), bad), (("--window-around", "-1"), bad),
                          (("--window-around", "1.5"), bad), (("--window-around", "99999999999999999999"), bad),
                          (("--window-around", "1,5"), "has 5 cameras, camera 5 was given"),
                          (("--window-around",), "requires a value but none was supplied"),
                          (("--window-around", "1", "--hops", "-1"), "Invalid value for '--hops"),
                          (("--window-around", "1", "--min-shared", "0"), "Invalid value for '--min-shared <K>'"),
                          (("--window-around", "1,2,3", "--max-cameras", "2"), "Invalid value for '--max-cameras <M>'"),
                          (("--hops", "2"), "--hops needs --window-around"), (("--min-shared", "2"), "--min-shared needs --window-around"),
                          (("--max-cameras", "2"), "--max-cameras needs --window-around"),
                          (("--window", "0:2", "--hops", "2"), "--hops needs --window-around")):
        r = subprocess.run([cli, "solve", str(src), out] + list(args), capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    assert not os.path.exists(out)
    for args, message in ((("--min-shared", "0"), "Invalid value for '--min-shared <K>'"), (("--min-shared",), "requires a value"),
                          (("--hops", "1"), "")):
        r = subprocess.run([cli, "covisibility", str(src)] + list(args), capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and message in r.stderr and r.stderr.strip(), (args, r.stderr)
    r = subprocess.run([cli, "covisibility"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "<FILE>" in r.stderr
