"""`city2ba noise --index-noise` without a GPU: the help and the usage comment name the flag, and a bad value -- or the flag
beside --gpus / --devices -- fails while the arguments are parsed, before a file is read or a device touched."""
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([entry.build_cli()] + list(args), capture_output=True, text=True, timeout=60)


def test_help_and_usage_comment_name_the_flag():
    out = _run("noise", "--help")
    assert out.returncode == 0
    assert "--index-noise <host|device> [host]" in out.stdout
    assert out.stdout.index("--index-noise") > out.stdout.index("--mismatch-chance")          # after the text the help already had
    head = open(os.path.join(ROOT, "city2ba_amd", "cli", "main.cpp")).read().split("#include", 1)[0]
    assert "[--index-noise host|device]" in head and head.index("--index-noise") < head.index("city2ba generate FILE OUT")


def test_bad_values_fail_before_the_device(tmp_path):
    a, b = str(tmp_path / "a.bal"), str(tmp_path / "b.bal")                  # neither exists: a parsed command would fail on the read
    bad = "Invalid value for '--index-noise <index-noise>': expected host or device"
    sharded = "--index-noise device runs on one GPU"
    for args, message in ((("--index-noise", "gpu"), bad), (("--index-noise", "Device"), bad), (("--index-noise", ""), bad),
                          (("--index-noise", "1"), bad), (("--index-noise",), "requires a value but none was supplied"),
                          (("--index-noise", "device", "--gpus", "2"), sharded), (("--gpus", "1", "--index-noise", "device"), sharded),
                          (("--index-noise", "device", "--devices", "0,1"), sharded),
                          (("--index-noise", "device", "--drop-features", "half"), "Invalid value for '--drop-features <drop-features>'")):
        r = _run("noise", a, b, "--drop-features", "0.5", *args) if "half" not in args else _run("noise", a, b, *args)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    assert not os.path.exists(b)
    for value in ("host", "device"):                         # parsed: the read fails, not the flag
        ok = _run("noise", a, b, "--drop-features", "0.5", "--index-noise", value)
        assert ok.returncode != 0 and "Invalid value" not in ok.stderr and "one GPU" not in ok.stderr, ok.stderr
    assert not os.path.exists(b)
