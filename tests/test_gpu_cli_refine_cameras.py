"""`city2ba refine --cameras` and `--alternate N` on the GPU: the file each writes is, byte for byte, the file Python writes after
BAProblem.refine_cameras / solve.alternate on the same input, the counts printed are those calls', and `refine` without the new
flags still writes what refine_points gives."""
import re
import subprocess

import pytest

import __graft_entry__ as entry
import _refinecamref as RC
from test_gpu_schur_step import env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
LINE = r"(?m)^refined (\d+) %s: (\d+) converged, (\d+) at the round limit; kept: (\d+) unobserved, (\d+) with a cost that is not finite, (\d+) constant$"
ORDER = ("moved", "converged", "max_rounds", "unobserved", "failed", "constant")


def _source(tmp_path):
    import city2ba_amd as c2b
    P = RC.dome(1e-3)
    src = str(tmp_path / "in.bbal")
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    ba.write(src)
    ba.close()
    return src


def _cli(tmp_path, src, name, *flags):
    out = str(tmp_path / name)
    run = subprocess.run([entry.build_cli(), "refine", src, out] + list(flags), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    return open(out, "rb").read(), run.stdout


@pytest.mark.parametrize("flags,kw,loss", [([], {}, None),
                                           (["--rounds", "4", "--lambda", "1e-3", "--loss", "cauchy", "--loss-scale", "0.05", "--function-tol", "1e-6"],
                                            dict(rounds=4, lam=1e-3, function_tol=1e-6), ("cauchy", 0.05))], ids=["default", "cauchy-4-rounds"])
def test_cli_refine_cameras_writes_what_python_writes(env, tmp_path, flags, kw, loss):
    import city2ba_amd as c2b
    src, out_py = _source(tmp_path), str(tmp_path / "py.bbal")
    got, stdout = _cli(tmp_path, src, "out.bbal", "--cameras", *flags)
    ba = c2b.BAProblem.from_file(src)
    if loss:
        ba.set_loss(*loss)
    counts = ba.refine_cameras(**kw)
    ba.write(out_py)
    ba.close()
    assert got == open(out_py, "rb").read()
    assert re.findall(LINE % "cameras", stdout) == [tuple(str(counts[k]) for k in ORDER)], stdout
    assert counts["moved"] > 80 and counts["unobserved"] == 1


def test_cli_alternate_and_the_plain_subcommand(env, tmp_path):
    import city2ba_amd as c2b
    from city2ba_amd import solve
    src, out_py, out_pts = _source(tmp_path), str(tmp_path / "py.bbal"), str(tmp_path / "pts.bbal")
    got, stdout = _cli(tmp_path, src, "out.bbal", "--alternate", "3", "--rounds", "2")
    ba = c2b.BAProblem.from_file(src)
    res = solve.alternate(ba, sweeps=3, camera_rounds=2, point_rounds=2)
    ba.write(out_py)
    ba.close()
    assert got == open(out_py, "rb").read() and res["sweeps"] == 3
    assert re.findall(LINE % "cameras", stdout) == [tuple(str(res["cameras"][k]) for k in ORDER)], stdout
    assert re.findall(LINE % "points", stdout) == [tuple(str(res["points"][k]) for k in ORDER)], stdout
    plain, stdout = _cli(tmp_path, src, "plain.bbal")                          # no new flag: the points alone, as before
    ba = c2b.BAProblem.from_file(src)
    counts = ba.refine_points()
    ba.write(out_pts)
    ba.close()
    assert plain == open(out_pts, "rb").read() != got
    assert re.findall(LINE % "points", stdout) == [tuple(str(counts[k]) for k in ORDER)] and not re.findall(LINE % "cameras", stdout)
