"""tools/benchkit.py, which every tools/bench_*.py script takes its timing, statistics, set-up and output from: the statistics
against values worked out by hand, emit's one line, every converted script's options (a child process with --help, which needs
no GPU), and on the GPU one script of each timing family end to end at a small size: the JSON has the key tree of the profile
committed for that script, every timing in it is a positive finite number, and what the run counted adds up.  No time is held
to a value."""
import importlib.util
import json
import math
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


def _benchkit():
    spec = importlib.util.spec_from_file_location("benchkit", os.path.join(TOOLS, "benchkit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


B = _benchkit()


# ---- statistics ------------------------------------------------------------------------------------------------------------
def test_the_two_medians_differ_on_an_even_count_and_agree_on_an_odd_one():
    even = [4.0, 1.0, 3.0, 2.0]
    assert B.median(even) == 2.5 and isinstance(B.median(even), float)
    assert B.upper_median(even) == 3.0
    assert even == [4.0, 1.0, 3.0, 2.0]                       # neither sorts its argument in place
    odd = [5.0, 1.0, 3.0]
    assert B.median(odd) == 3.0 and B.upper_median(odd) == 3.0
    assert B.median([7.5]) == 7.5 and B.upper_median([7.5]) == 7.5


def test_spread_is_min_and_max_rounded():
    assert B.spread([3.0, 1.234, 4.128, 2.0], 2) == [1.23, 4.13]
    assert B.spread([3.0, 1.234, 4.128, 2.0], 1) == [1.2, 4.1]
    assert B.spread([0.0123456], 4) == [0.0123, 0.0123]


def test_us_record_is_the_upper_median_and_the_minimum_to_a_tenth():
    rec = B.us_record([10.04, 30.06, 20.0, 40.0])
    assert rec == {"median_us": 30.1, "min_us": 10.0} and list(rec) == ["median_us", "min_us"]
    assert B.us_record([2.26, 2.24, 2.25 + 1e-9]) == {"median_us": 2.3, "min_us": 2.2}


def test_frac_of_peak_is_bytes_over_time_over_8_terabytes_per_second():
    assert B.HBM_PEAK_BYTES_PER_S == 8.0e12
    assert abs(B.frac_of_peak(8.0e6, 1.0) - 1.0) < 1e-12      # 8 MB in a microsecond is the peak
    assert abs(B.frac_of_peak(4.0e6, 2.0) - 0.25) < 1e-12
    # the two passes of profiles/normal_equations_bench_blocks128.json: its bytes and medians give its fractions
    assert round(B.frac_of_peak(1057097560, 1027.4), 4) == 0.1286
    assert round(B.frac_of_peak(859547856, 406.4), 4) == 0.2644


# ---- emit ------------------------------------------------------------------------------------------------------------------
def test_emit_writes_one_line_to_stdout_and_the_same_line_to_the_file(tmp_path, capsys):
    result = dict(bench="x", n=3, nested=dict(b=[1.5, 2.5], a=None), flag=True)
    path = tmp_path / "sub" / "out.json"                      # (a directory that does not exist yet is made)
    B.emit(result, str(path))
    printed = capsys.readouterr().out
    assert printed.count("\n") == 1 and printed.endswith("\n")
    assert path.read_text() == printed
    assert json.loads(printed) == result and list(json.loads(printed)) == ["bench", "n", "nested", "flag"]


def test_emit_without_a_path_only_prints(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    B.emit({"a": 1})
    B.emit({"a": 2}, "")
    B.emit({"a": 3}, None)
    assert capsys.readouterr().out == '{"a": 1}\n{"a": 2}\n{"a": 3}\n'
    assert os.listdir(tmp_path) == []


# ---- every converted script's options ------------------------------------------------------------------------------------------
OPTIONS = {
    "bench_triangulate.py": "blocks sigma point-std min-angle launches repeats out",
    "bench_triangulate_robust.py": "blocks sigma point-std mismatch min-angle max-error min-inliers max-hypotheses launches repeats out",
    "bench_resect.py": "blocks sigma rotation-std translation-std min-points min-gap launches repeats out",
    "bench_resect_robust.py": "blocks sigma rotation-std translation-std mismatch max-error min-inliers min-gap max-hypotheses launches repeats out",
    "bench_refine.py": "blocks sigma point-std lam launches repeats iterations out",
    "bench_refine_cameras.py": "blocks sigma translation-std rotation-std lam launches repeats out",
    "bench_rematch.py": "blocks join mismatch seed radius max-error min-fits repeats out",
    "bench_merge.py": "blocks split seed radius max-error rounds repeats out",
    "bench_filter.py": "blocks sigma mismatch repeats out",
    "bench_lm.py": "blocks iterations lam repeats out",
    "bench_window.py": "blocks sigma point-std repeats size iterations out",
    "bench_index_noise.py": "blocks repeats seed dir out",
    "bench_normal.py": "blocks reps warmup",
    "bench_schur.py": "blocks reps warmup loss loss-scale preconditioner constant to-tol tol-max-iters",
    "bench_priors.py": "blocks reps warmup rounds sigma drift tol-max-iters lm-iterations gradient-drop out",
    "bench_align.py": "blocks repeats out",
    "bench_covisibility.py": "blocks min-shared repeats size seed no-host out",
}


@pytest.mark.parametrize("script", sorted(OPTIONS))
def test_help_lists_the_scripts_options_without_a_gpu(script):
    p = subprocess.run([sys.executable, os.path.join(TOOLS, script), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    # the options' own entries: an indented line that opens with the option (or with "-h, --help")
    listed = re.findall(r"(?m)^\s+(?:-h, )?--([a-z][a-z0-9-]*)", p.stdout)
    assert listed == ["help"] + OPTIONS[script].split(), listed


# ---- one script of each timing family, on the GPU -----------------------------------------------------------------------------------
# --blocks 8 with two repeats (and two launches per window where there is the option): the culled grid is not empty there (2 860
# of its 2 880 cameras stay), and every script's own counts and comparisons hold.  bench_normal.py names its repeats --reps and has a --warmup.
FAMILIES = {
    "bench_triangulate.py": dict(args=["--blocks", "8", "--repeats", "2", "--launches", "2"], profile="triangulate_bench_blocks128.json",
                                 timings=["kernel_us", "spread_us", "ratio_triangulate_over_normal_points"]),              # event window
    "bench_normal.py": dict(args=["--blocks", "8", "--reps", "2", "--warmup", "1"], profile="normal_equations_bench_blocks128.json",
                            timings=["transpose", "cameras", "points", "both_passes_us", "both_frac_of_8TBs", "step_us", "both_over_step"]),   # event per call
    "bench_filter.py": dict(args=["--blocks", "8", "--repeats", "2"], profile="filter_observations_bench_blocks128.json",
                            timings=["filter_ms", "step_after_ms"]),                                                        # host clock
}


def _key_tree(x):
    """keys, their order and their nesting; values dropped"""
    return [(k, _key_tree(v)) for k, v in x.items()] if isinstance(x, dict) else None


def _numbers(x):
    if isinstance(x, dict):
        x = list(x.values())
    if isinstance(x, list):
        return [v for item in x for v in _numbers(item)]
    return [x]


@pytest.mark.gpu
@pytest.mark.parametrize("script", sorted(FAMILIES))
def test_a_script_of_each_timing_family_prints_its_profiles_key_tree(script):
    case = FAMILIES[script]
    p = subprocess.run([sys.executable, os.path.join(TOOLS, script)] + case["args"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-3000:]
    out = json.loads(lines[0])
    print(lines[0])
    with open(os.path.join(ROOT, "profiles", case["profile"])) as fh:
        assert _key_tree(out) == _key_tree(json.load(fh))
    assert out["blocks"] == 8 and out["n_cam"] > 0 and out["n_pts"] > 0 and out["n_obs"] > 0
    for key in case["timings"]:
        values = _numbers(out[key])
        assert values and all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v > 0 for v in values), (key, out[key])
    if "counts" in out:                                       # the status of every point, counted
        assert sum(out["counts"].values()) == out["n_pts"], out["counts"]
    if "same_lists" in out:
        assert out["same_lists"] is True and 0 < out["removed"] < out["n_obs"]
