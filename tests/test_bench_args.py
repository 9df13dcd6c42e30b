"""bench.py without a device: its options, its argument checks (made before anything touches a GPU), and the
--dump-outputs sample on host tensors -- fixed by its seed, the rows of the sampled observations, under 64 MB."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([sys.executable, "bench.py"] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_options_and_argument_checks():
    p = _run("--help")
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout, p.stderr
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        p = _run(*bad)
        assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, (bad, p.stderr)


def test_output_sample_is_seeded_and_takes_the_sampled_rows(tmp_path):
    import torch
    import bench
    for n_total in (5000, 19_302_494):
        n = min(n_total, 600_000)                                 # a shard holding the observations [lo, lo + n)
        lo = n_total - n
        r = torch.arange(n * 2, dtype=torch.float64).reshape(n, 2)
        Jc = torch.arange(n * 18, dtype=torch.float64).reshape(n, 18)
        Jp = torch.arange(n * 6, dtype=torch.float64).reshape(n, 6)
        sh = {"n_obs_total": n_total, "obs_base": lo, "n_obs": n}
        e = torch.tensor(6.25, dtype=torch.float64)
        a = bench.output_sample(sh, r, Jc, Jp, e, False, 1)
        b = bench.output_sample(sh, r, Jc, Jp, e, False, 1)
        for name in a:
            assert a[name].dtype == np.float64 and np.array_equal(a[name], b[name]), name
        idx = a["observation_index"].astype(np.int64)
        assert np.all(np.diff(idx) > 0) and idx.min() >= lo and idx.max() < n_total
        if n_total <= bench.DUMP_ROWS:
            assert len(idx) == n_total
        loc = idx - lo
        assert np.array_equal(a["residual"], r.numpy()[loc]) and np.array_equal(a["jacobian_camera"], Jc.numpy()[loc])
        assert np.array_equal(a["jacobian_point"], Jp.numpy()[loc])
        assert a["error_sum"].tolist() == [6.25] and a["total_l2_error"].tolist() == [2.5]
    # the whole-list sample of the headline size fits the 64 MB cap
    assert bench.DUMP_ROWS * (2 + 18 + 6 + 1) * 8 + 2 * 8 <= 64 << 20
    bench.write_outputs(str(tmp_path / "d"), a)
    back = {f[:-4]: np.load(str(tmp_path / "d" / f)) for f in os.listdir(str(tmp_path / "d"))}
    assert sorted(back) == sorted(a) and all(np.array_equal(back[k], a[k]) for k in a)
