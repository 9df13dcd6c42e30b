"""bench.py's plain run and --dump-outputs: the plain line carries the headline and nothing that takes runs of its own
(those come with --full), and the dumped sample is what the timed step computed -- the rows of the sampled observations
equal the CPU oracle's on the same seeded inputs, and a second run with the same arguments dumps the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--blocks", "32", "--steps", "7", "--warmup", "2"]
NAMES = ("residual", "jacobian_camera", "jacobian_point", "observation_index", "error_sum", "total_l2_error")


def _bench(extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "C2B_DIST_BACKEND", "C2B_SHARE_GPU"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "bench.py"] + ARGS + extra, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-3000:]
    return json.loads(lines[0])


def _load(d):
    return {name: np.load(os.path.join(d, name + ".npy")) for name in NAMES}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump_a")
    return _bench(["--dump-outputs", str(d)]), str(d)


def test_plain_line_is_the_headline(plain):
    out, _ = plain
    assert out["metric"] == "million observations/sec (project+Jacobian)" and out["unit"] == "Mobs/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f64" and out["n_gpus"] == 1
    assert out["steps"] == 7 and out["warmup"] == 2
    assert out["value"] > 0 and out["ms_per_step"] > 0
    n = out["config"]["n_observations"]
    assert abs(out["value"] - n / (out["ms_per_step"] * 1e3)) <= 1e-3 * out["value"]      # value and ms_per_step: one step
    assert out["roofline"]["kernel_avg_us"] > 0 and out["roofline"]["frac"] > 0              # events inside the region
    # nothing that takes runs of its own
    assert out["cpu_baseline"] is None
    for key in ("other_configs", "value_caches_swept", "value_first_allocation"):
        assert key not in out, key
    assert out["roofline"]["kernel_us_first_allocation"] is None
    assert not any(k.startswith("same_run_") for k in out["roofline"])


def test_dumped_outputs_are_the_last_steps_and_match_the_oracle(plain):
    import argparse
    import torch
    import bench
    import oracle as O
    out, d = plain
    got = _load(d)
    assert sum(os.path.getsize(os.path.join(d, name + ".npy")) for name in NAMES) <= 64 << 20
    assert all(a.dtype == np.float64 for a in got.values())
    idx = got["observation_index"]
    n_total = out["config"]["n_observations"]
    k = min(n_total, bench.DUMP_ROWS)
    assert idx.shape == (k,) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n_total
    assert got["residual"].shape == (k, 2) and got["jacobian_camera"].shape == (k, 18) and got["jacobian_point"].shape == (k, 6)
    assert got["total_l2_error"][0] == out["config"]["total_L2_error"]
    assert abs(got["error_sum"][0] ** 0.5 - got["total_l2_error"][0]) <= 1e-15 * got["total_l2_error"][0]

    # the same seeded inputs, rebuilt in this process, through the CPU oracle
    dev = torch.device("cuda", 0)
    sh = bench.build_shard(argparse.Namespace(blocks=32), 0, 1, dev)
    assert sh["n_obs"] == n_total
    row_ptr = sh["rows"].row_ptr.cpu().numpy().astype(np.uint64)
    pt_idx = sh["pt_idx"].cpu().numpy().astype(np.uint64)
    pts = np.ascontiguousarray(sh["pts4"][:, :3].cpu().numpy())
    cams15, uv = sh["cam15"].cpu().numpy(), sh["uv"].cpu().numpy()
    r0, Jc0, Jp0 = O.residual_jacobian(cams15, pts, row_ptr, pt_idx, uv)
    sel = idx.astype(np.int64)
    assert np.max(np.abs(got["residual"] - r0[sel])) < 1e-9 * max(1.0, float(np.max(np.abs(r0[sel]))))
    scale = max(1.0, float(np.max(np.abs(Jc0[sel]))))
    assert np.max(np.abs(got["jacobian_camera"] - Jc0[sel])) / scale < 1e-6
    assert np.max(np.abs(got["jacobian_point"] - Jp0[sel])) / scale < 1e-6
    e0 = O.total_reprojection_error(cams15, pts, row_ptr, pt_idx, uv, 2.0)
    assert abs(got["total_l2_error"][0] - e0) <= 1e-9 * e0


def test_same_arguments_dump_the_same_outputs(plain, tmp_path):
    _, d = plain
    _bench(["--dump-outputs", str(tmp_path)])
    a, b = _load(d), _load(str(tmp_path))
    for name in ("residual", "jacobian_camera", "jacobian_point", "observation_index"):
        assert np.array_equal(a[name], b[name]), name
    # the folded sum: the launch shape follows the measured store rate of the kept set, so its order may differ
    assert abs(a["error_sum"][0] - b["error_sum"][0]) <= 1e-12 * a["error_sum"][0]


def test_full_line_carries_what_the_plain_one_leaves_out():
    out = _bench(["--full", "--cpu-seconds", "1"])
    assert out["steps"] == 7 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["value_caches_swept"] > 0 and out["value_first_allocation"] > 0
    assert out["roofline"]["kernel_us_first_allocation"] > 0 and out["roofline"]["same_run_store_GBs"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["value_all_cores"] > 0
