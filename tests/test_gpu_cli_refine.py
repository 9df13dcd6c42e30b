"""`city2ba refine` and `city2ba solve --inner-iterations` on the GPU: the file each writes is, byte for byte, the file Python
writes after BAProblem.refine_points / levenberg_marquardt_device(inner_iterations=...) on the same input, and the counts
`refine` prints are that call's."""
import re
import subprocess

import pytest

import __graft_entry__ as entry
import _triangref as T
from test_gpu_schur_step import env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu


def _source(tmp_path):
    import city2ba_amd as c2b
    P = T.dome_case(False, 1e-3)
    src = str(tmp_path / "in.bbal")
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    ba.write(src)
    ba.close()
    return src


@pytest.mark.parametrize("flags,kw,loss", [([], {}, None),
                                           (["--rounds", "4", "--lambda", "1e-3", "--loss", "cauchy", "--loss-scale", "0.05", "--function-tol", "1e-6"],
                                            dict(rounds=4, lam=1e-3, function_tol=1e-6), ("cauchy", 0.05))], ids=["default", "cauchy-4-rounds"])
def test_cli_refine_writes_what_python_writes(env, tmp_path, flags, kw, loss):
    import city2ba_amd as c2b
    src, out_cli, out_py = _source(tmp_path), str(tmp_path / "out.bbal"), str(tmp_path / "py.bbal")
    run = subprocess.run([entry.build_cli(), "refine", src, out_cli] + flags, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    ba = c2b.BAProblem.from_file(src)
    if loss:
        ba.set_loss(*loss)
    counts = ba.refine_points(**kw)
    ba.write(out_py)
    ba.close()
    assert open(out_cli, "rb").read() == open(out_py, "rb").read()
    m = re.findall(r"(?m)^refined (\d+) points: (\d+) converged, (\d+) at the round limit; kept: (\d+) unobserved, (\d+) with a cost that is not finite, (\d+) constant$",
                   run.stdout)
    assert m == [tuple(str(counts[k]) for k in ("moved", "converged", "max_rounds", "unobserved", "failed", "constant"))], run.stdout
    assert counts["moved"] > 300 and counts["unobserved"] == 20
    if loss:
        assert counts["converged"] > 0


def test_cli_solve_with_inner_iterations_writes_what_the_device_loop_gives(env, tmp_path):
    import city2ba_amd as c2b
    from city2ba_amd import solve
    src, out_cli, out_py, out_plain = _source(tmp_path), str(tmp_path / "out.bbal"), str(tmp_path / "py.bbal"), str(tmp_path / "plain.bbal")
    run = subprocess.run([entry.build_cli(), "solve", src, out_cli, "--iterations", "4", "--inner-iterations", "2"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    ba = c2b.BAProblem.from_file(src)
    h, s = solve.levenberg_marquardt_device(ba, 4, inner_iterations=2)
    ba.write(out_py)
    ba.close()
    ba = c2b.BAProblem.from_file(src)
    solve.levenberg_marquardt_device(ba, 4)
    ba.write(out_plain)
    ba.close()
    assert open(out_cli, "rb").read() == open(out_py, "rb").read() != open(out_plain, "rb").read()
    m = re.search(r"(?m)^Termination: iteration limit reached after 4 iterations; cost (\S+) -> (\S+)$", run.stdout)
    assert m and float(m.group(1)) == s["initial_cost"] and float(m.group(2)) == s["final_cost"], run.stdout
