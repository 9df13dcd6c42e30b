"""`city2ba solve --window LO:HI [--no-halo]` without a GPU: the help names both flags, the usage comment lists them, and
every bad range is refused before a device is touched -- a malformed range, LO >= HI, HI beyond the file's camera count (read
from its first line alone), --no-halo without a window."""
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_names_the_flags():
    cli = entry.build_cli()
    out = subprocess.run([cli, "solve", "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    for text in ("--window <LO:HI>", "--no-halo", "held constant", "the whole problem is written"):
        assert text in out.stdout, text
    assert out.stdout.index("--window <LO:HI>") > out.stdout.index("--inner-iterations <N>")           # after the text the help already had
    head = open(os.path.join(ROOT, "city2ba_amd", "cli", "main.cpp")).read().split("#include", 1)[0]
    assert "[--window LO:HI [--no-halo]]" in head


def test_bad_ranges_are_refused_before_the_device(tmp_path):
    cli = entry.build_cli()
    src, out = tmp_path / "in.bal", str(tmp_path / "out.bal")
    src.write_text("5 7 0\n")                                # the counts alone: a parsed command would fail on the read
    bad = "Invalid value for '--window <LO:HI>': expected two integers LO:HI with 0 <= LO < HI"
    for args, message in ((("--window", "3"), bad), (("--window", "3:"), bad), (("--window", ":3"), bad), (("--window", "a:b"), bad),
                          (("--window", "1:2:3"), bad), (("--window", "-1:3"), bad), (("--window", "1.5:3"), bad),
                          (("--window", "3:3"), bad), (("--window", "4:2"), bad), (("--window", "0:99999999999999999999"), bad),
                          (("--window", "0:6"), "has 5 cameras, the window ends at 6"),
                          (("--window",), "requires a value but none was supplied"),
                          (("--no-halo",), "--no-halo needs --window <LO:HI>")):
        r = subprocess.run([cli, "solve", str(src), out] + list(args), capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    assert not os.path.exists(out)
    missing = subprocess.run([cli, "solve", str(tmp_path / "none.bal"), out, "--window", "0:2"], capture_output=True, text=True, timeout=60)
    assert missing.returncode != 0 and "Could not open" in missing.stderr
