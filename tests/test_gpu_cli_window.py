"""`city2ba solve IN OUT --window 37:101 [--no-halo]` on the device writes the file the Python calls give, byte for byte:
BAProblem.from_file, solve.solve_window(range(37, 101)) with the command's defaults, write."""
import subprocess

import numpy as np
import pytest

import _subsetref as SR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("halo", [True, False], ids=["halo", "nohalo"])
def test_the_command_writes_what_solve_window_writes(tmp_path, halo):
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd as c2b
    import oracle as O
    from city2ba_amd import solve as S
    cli = entry.build_cli()
    cams, pts, row_ptr, pt_idx, uv = SR.locality_grid()
    bal9 = O.camera_to_bal(cams)
    rng = np.random.default_rng(9)
    bal9[:, :6] += rng.normal(scale=2e-3, size=(len(bal9), 6))
    pts = pts + rng.normal(scale=2e-3, size=pts.shape)
    src, by_cli, by_py = (str(tmp_path / n) for n in ("in.bbal", "cli.bbal", "py.bbal"))
    from city2ba_amd.baproblem import write_bal
    write_bal(src, bal9, pts, row_ptr, pt_idx, uv)
    r = subprocess.run([cli, "solve", src, by_cli, "--window", "37:101", "--iterations", "4"] + ([] if halo else ["--no-halo"]),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = (140, 260, 1470) if halo else (64, 260, 758)
    assert "window 37:101: %d cameras, %d points, %d observations" % want in r.stdout
    assert "written back: 64 cameras, %d points" % (260 if halo else 260 - 179) in r.stdout
    ba = c2b.BAProblem.from_file(src)
    s = S.solve_window(ba, range(37, 101), halo=halo, iterations=4)
    assert (s["cameras"], s["points"], s["observations"]) == want and s["final_cost"] < s["initial_cost"]
    ba.write(by_py)
    ba.close()
    a, b = open(by_cli, "rb").read(), open(by_py, "rb").read()
    assert a == b and a != open(src, "rb").read()
