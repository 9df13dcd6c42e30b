"""`city2ba solve` end to end on the GPU: synthetic, then noise, then solve, each its own child process under its own
time limit; the solved file holds, bit for bit, the cameras and points city2ba_amd.solve.levenberg_marquardt_device leaves
on the same input with the same options, and the printed costs are the history's."""
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


@pytest.mark.parametrize("ext,flags,kw", [
    ("bal", [], {}),
    ("bbal", ["--loss", "huber", "--fix-intrinsics"], dict(loss="huber")),
], ids=["bal", "bbal-huber-fixed-intrinsics"])
def test_solve_matches_the_device_loop(env, tmp_path, ext, flags, kw):
    import city2ba_amd as c2b
    from city2ba_amd import solve
    from city2ba_amd.baproblem import read_bal
    clean, noisy, solved = (tmp_path / ("%s.%s" % (n, ext)) for n in ("clean", "noisy", "solved"))
    _run(["synthetic", clean, "--blocks", 2], 120)
    _run(["noise", clean, noisy, "--point-std", "1e-2", "--observation-std", "1e-3", "--seed", 3], 120)
    text = _run(["solve", noisy, solved, "--iterations", 5] + flags, 120)
    assert os.path.getsize(solved) > 0

    ba = c2b.BAProblem.from_file(str(noisy))
    if "--fix-intrinsics" in flags:
        kw = dict(kw, constant=(np.full(ba.num_cameras(), solve.INTRINSICS, dtype=np.uint16), None))
    h, s = solve.levenberg_marquardt_device(ba, 5, **kw)
    bal9, pts, row_ptr, pt_idx, uv = read_bal(str(solved))
    assert _bits(bal9, ba.cameras_bal()) and _bits(pts, ba.points())
    assert _bits(row_ptr, ba.row_ptr) and _bits(pt_idx, ba.pt_idx) and _bits(uv, ba.observations())
    if "--fix-intrinsics" in flags:
        assert _bits(bal9[:, 6:], read_bal(str(noisy))[0][:, 6:])
    ba.close()

    lines = re.findall(r"(?m)^iteration (\d+): cost (\S+) lambda (\S+) (accepted|rejected) pcg (\d+)$", text)
    assert len(lines) == len(h) == 5, text
    for k, (i, cost, lam, acc, pcg) in enumerate(lines):
        assert int(i) == k and float(cost) == h[k]["cost"] and (acc == "accepted") == h[k]["accepted"] and int(pcg) == h[k]["pcg_iterations"]
        assert float(lam) == float("%.6e" % h[k]["lam"])
    m = re.search(r"(?m)^Termination: iteration limit reached after 5 iterations; cost (\S+) -> (\S+)$", text)
    assert m and float(m.group(1)) == s["initial_cost"] and float(m.group(2)) == s["final_cost"], text
    assert s["final_cost"] < s["initial_cost"]
