"""tools/bench_dense_schur.py as tests/test_tools_bench_schur_explicit.py holds its sibling: the help lists exactly its options
without a GPU, and on the GPU a small window prints one JSON line with the keys DESIGN 4.23's tables are made from."""
import json
import os
import re
import subprocess
import sys

import pytest

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bench_dense_schur.py")
OPTIONS = "blocks window halo sigma point-std reps warmup iterations out"
KEYS = {"bench", "blocks", "window", "halo", "n_cam", "n_pts", "n_obs", "n_edges", "order", "padded_order", "linear_solver_bytes", "lambda", "level0",
        "solve_step", "lm"}
STEPS = {"cholesky", "pcg_implicit_default", "pcg_explicit_default", "pcg_implicit_1e-10", "pcg_explicit_1e-10"}


def test_help_lists_the_options_without_a_gpu():
    p = subprocess.run([sys.executable, TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    listed = re.findall(r"(?m)^\s+(?:-h, )?--([a-z][a-z0-9-]*)", p.stdout)
    assert listed == ["help"] + OPTIONS.split(), listed


@pytest.mark.gpu
def test_a_small_window_prints_the_line():
    p = subprocess.run([sys.executable, TOOL, "--blocks", "2", "--window", "24", "--reps", "2", "--iterations", "3"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(out) == KEYS and set(out["solve_step"]) == STEPS and set(out["lm"]) == {"cholesky", "pcg_default"}, sorted(out)
    assert out["n_cam"] == 24 and out["order"] == 216 and out["padded_order"] == 256
    assert out["level0"]["factor"]["launches"] == 10 and out["level0"]["factor"]["info"] == 0 and out["level0"]["factor"]["median_us"] > 0
    assert out["solve_step"]["cholesky"]["iterations"] == 0 and out["solve_step"]["cholesky"]["status"] == 0
    assert out["lm"]["cholesky"]["pcg_iterations"] == 0 and out["lm"]["pcg_default"]["pcg_iterations"] > 0
