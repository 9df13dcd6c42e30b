"""`city2ba solve --prior-from` end to end on the GPU: synthetic, noise, solve, each its own child process under its own
time limit; the solved file holds, bit for bit, what city2ba_amd.solve.levenberg_marquardt_device leaves on the same input
with the same priors, and the printed costs are the history's (test_gpu_cli_solve's criterion)."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from test_gpu_schur_step import _bits, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu


def _run(args, limit):
    """one child process; the chain stops at the first status that is not 0"""
    out = subprocess.run([entry.build_cli()] + [str(a) for a in args], capture_output=True, text=True, timeout=limit)
    assert out.returncode == 0, (args, out.returncode, out.stdout, out.stderr)
    return out.stdout


def test_solve_with_priors_matches_the_device_loop(env, tmp_path):
    import city2ba_amd as c2b
    from city2ba_amd import solve
    from city2ba_amd.baproblem import read_bal
    clean, noisy, solved = (tmp_path / ("%s.bal" % n) for n in ("clean", "noisy", "solved"))
    _run(["synthetic", clean, "--blocks", 2], 120)
    _run(["noise", clean, noisy, "--point-std", "1e-2", "--observation-std", "1e-3", "--seed", 3], 120)
    flags = ["--prior-from", clean, "--prior-center-sigma", "0.5,0.25,1", "--prior-intrinsics-sigma", "0.1,0.01,0.01",
             "--prior-point-sigma", "2", "--prior-point-every", "7"]
    text = _run(["solve", noisy, solved, "--iterations", 5] + flags, 120)
    assert os.path.getsize(solved) > 0

    target = c2b.BAProblem.from_file(str(clean))
    ba = c2b.BAProblem.from_file(str(noisy))
    xw = np.zeros((ba.num_points(), 3))
    xw[::7] = 1.0 / 2
    priors = dict(camera_centers=target._camera_centers(), camera_center_weights=[1 / 0.5, 1 / 0.25, 1.0],
                  intrinsics=target.cameras_bal()[:, 6:9].copy(), intrinsics_weights=[1 / 0.1, 1 / 0.01, 1 / 0.01],
                  points=target.points(), point_weights=xw)
    target.close()
    h, s = solve.levenberg_marquardt_device(ba, 5, priors=priors)
    assert ba.priors["active"] == (ba.num_cameras(), ba.num_cameras(), len(xw[::7]))
    bal9, pts, row_ptr, pt_idx, uv = read_bal(str(solved))
    assert _bits(bal9, ba.cameras_bal()) and _bits(pts, ba.points())
    assert _bits(row_ptr, ba.row_ptr) and _bits(pt_idx, ba.pt_idx) and _bits(uv, ba.observations())
    plain = c2b.BAProblem.from_file(str(noisy))
    solve.levenberg_marquardt_device(plain, 5)
    assert not (_bits(plain.cameras_bal(), bal9) and _bits(plain.points(), pts))     # the priors did something
    assert any(e["accepted"] for e in h)
    plain.close()
    ba.close()

    lines = re.findall(r"(?m)^iteration (\d+): cost (\S+) lambda (\S+) (accepted|rejected) pcg (\d+)$", text)
    assert len(lines) == len(h) == 5, text
    for k, (i, cost, lam, acc, pcg) in enumerate(lines):
        assert int(i) == k and float(cost) == h[k]["cost"] and (acc == "accepted") == h[k]["accepted"] and int(pcg) == h[k]["pcg_iterations"]
        assert float(lam) == float("%.6e" % h[k]["lam"])
    m = re.search(r"(?m)^Termination: iteration limit reached after 5 iterations; cost (\S+) -> (\S+)$", text)
    assert m and float(m.group(1)) == s["initial_cost"] and float(m.group(2)) == s["final_cost"], text
    assert s["final_cost"] < s["initial_cost"]
