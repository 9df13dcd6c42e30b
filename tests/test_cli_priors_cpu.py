"""`city2ba solve --prior-*` without a device: the help lists the flags, and every argument error -- a sigma flag without
--prior-from, a sigma that is not > 0, a malformed list, a count mismatch between the two files -- comes from the parser
before anything touches a GPU."""
import subprocess

import __graft_entry__ as entry

FLAGS = ("--prior-from", "--prior-center-sigma", "--prior-intrinsics-sigma", "--prior-point-sigma", "--prior-point-every")


def _run(*args):
    return subprocess.run([entry.build_cli()] + list(args), capture_output=True, text=True, timeout=60)


def _bal(path, n_cam, n_pts):
    """a .bal header is all the parser looks at before the device: counts, then nothing it reads"""
    path.write_text("%d %d 0\n" % (n_cam, n_pts))
    return str(path)


def test_help_lists_the_prior_flags():
    out = _run("solve", "--help")
    assert out.returncode == 0
    for flag in FLAGS:
        assert flag in out.stdout, flag


def test_prior_argument_errors_need_no_device(tmp_path):
    a, b = _bal(tmp_path / "a.bal", 7, 30), str(tmp_path / "out.bal")
    same, fewer_cams, fewer_pts = _bal(tmp_path / "t.bal", 7, 30), _bal(tmp_path / "c.bal", 6, 30), _bal(tmp_path / "p.bal", 7, 29)
    bb = tmp_path / "t.bbal"
    bb.write_bytes((6).to_bytes(8, "big") + (30).to_bytes(8, "big") + (0).to_bytes(8, "big"))
    cases = (
        (("--prior-center-sigma", "0.1"), "--prior-center-sigma needs --prior-from <FILE>"),
        (("--prior-intrinsics-sigma", "1,1,1"), "--prior-intrinsics-sigma needs --prior-from <FILE>"),
        (("--prior-point-sigma", "0.1"), "--prior-point-sigma needs --prior-from <FILE>"),
        (("--prior-point-every", "3"), "--prior-point-every needs --prior-from <FILE>"),
        (("--prior-from", same), "--prior-from <FILE> needs at least one of"),
        (("--prior-from", same, "--prior-center-sigma", "0"), "Invalid value for '--prior-center-sigma <S|SX,SY,SZ>'"),
        (("--prior-from", same, "--prior-center-sigma", "-1"), "Invalid value for '--prior-center-sigma <S|SX,SY,SZ>'"),
        (("--prior-from", same, "--prior-center-sigma", "1,2"), "Invalid value for '--prior-center-sigma <S|SX,SY,SZ>'"),
        (("--prior-from", same, "--prior-center-sigma", "1,x,2"), "Invalid value for '--prior-center-sigma <S|SX,SY,SZ>'"),
        (("--prior-from", same, "--prior-center-sigma", "nan"), "Invalid value for '--prior-center-sigma <S|SX,SY,SZ>'"),
        (("--prior-from", same, "--prior-intrinsics-sigma", "1"), "Invalid value for '--prior-intrinsics-sigma <SF,SK1,SK2>'"),
        (("--prior-from", same, "--prior-intrinsics-sigma", "1,0,1"), "Invalid value for '--prior-intrinsics-sigma <SF,SK1,SK2>'"),
        (("--prior-from", same, "--prior-point-sigma", "1,1,1"), "Invalid value for '--prior-point-sigma <S>'"),
        (("--prior-from", same, "--prior-point-sigma", "0"), "Invalid value for '--prior-point-sigma <S>'"),
        (("--prior-from", same, "--prior-center-sigma", "1", "--prior-point-every", "2"), "--prior-point-every needs --prior-point-sigma <S>"),
        (("--prior-from", same, "--prior-point-sigma", "1", "--prior-point-every", "0"), "Invalid value for '--prior-point-every <N>'"),
        (("--prior-from", fewer_cams, "--prior-center-sigma", "1"), "--prior-from: %s has 6 cameras, %s has 7" % (fewer_cams, a)),
        (("--prior-from", str(bb), "--prior-center-sigma", "1"), "--prior-from: %s has 6 cameras, %s has 7" % (bb, a)),
        (("--prior-from", fewer_pts, "--prior-point-sigma", "1"), "--prior-from: %s has 29 points, %s has 30" % (fewer_pts, a)),
        (("--prior-from", str(tmp_path / "missing.bal"), "--prior-center-sigma", "1"), "Could not open"),
    )
    for extra, message in cases:
        out = _run("solve", a, b, *extra)
        assert out.returncode == 1 and out.stderr.startswith("Error: " + message), (extra, out.returncode, out.stderr)
        assert "HIP" not in out.stderr and "device" not in out.stderr, out.stderr
