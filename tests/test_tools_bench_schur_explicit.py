"""tools/bench_schur_explicit.py as tests/test_tools_benchkit.py holds its siblings: the help lists exactly its options without a
GPU, and on the GPU a small grid prints one JSON line with the keys DESIGN 4.22's table is made from, under either setting."""
import json
import os
import re
import subprocess
import sys

import pytest

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bench_schur_explicit.py")
OPTIONS = "blocks points-per-block schur preconditioner reps warmup to-tol tol-max-iters"
SOLVE_KEYS = {"blocks", "points_per_block", "schur", "preconditioner", "n_obs", "n_cam", "n_pts", "lambda", "solve_0_iterations",
              "solve_25_iterations", "pcg_iteration_ms", "info_25", "to_rel_tol_0.01", "to_rel_tol_0.0001"}
EXPLICIT_KEYS = {"n_edges", "obs_per_edge", "pattern_build_ms", "schur_bytes", "schur_y_pass", "schur_blocks_pass", "schur_spmv_pass"}


def test_help_lists_the_options_without_a_gpu():
    p = subprocess.run([sys.executable, TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    listed = re.findall(r"(?m)^\s+(?:-h, )?--([a-z][a-z0-9-]*)", p.stdout)
    assert listed == ["help"] + OPTIONS.split(), listed


@pytest.mark.gpu
@pytest.mark.parametrize("schur", ["implicit", "explicit"])
def test_a_small_grid_prints_the_line(schur):
    p = subprocess.run([sys.executable, TOOL, "--blocks", "4", "--points-per-block", "30", "--schur", schur, "--reps", "2", "--to-tol",
                        "--tol-max-iters", "50"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(out) == SOLVE_KEYS | (EXPLICIT_KEYS if schur == "explicit" else set()), sorted(out)
    assert out["schur"] == schur and out["points_per_block"] == 30 and out["info_25"]["iterations"] == 25
    if schur == "explicit":
        assert out["n_edges"] > 0 and out["schur_bytes"] == 648 * (out["n_edges"] + out["n_cam"]) + 216 * out["n_obs"]
        for k in ("schur_y_pass", "schur_blocks_pass", "schur_spmv_pass"):
            assert out[k]["median_us"] > 0 and out[k]["algorithmic_bytes"] > 0
