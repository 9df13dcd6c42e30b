"""`city2ba compare` on the device: on two small .bbal files it prints the numbers of BAProblem.align, and --apply writes a file whose
own comparison against REF has the identity transform within the fit's bounds."""
import json
import subprocess

import numpy as np
import pytest

import _alignref as A
from _problems import dome_problem

pytestmark = pytest.mark.gpu
U = A.U


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd as c2b
    import oracle as O
    assert c2b.device_count() > 0
    d = dome_problem(seed=0)
    tmp = tmp_path_factory.mktemp("compare")
    truth = c2b.BAProblem.from_bal(d["true_bal9"], d["true_pts"], d["row_ptr"], d["pt_idx"], d["uv"])
    mc, mp = A.apply(O.camera_from_bal(d["bal9"]), d["pts"], 1.0 / A.S0, A.R0.T, [3.0, -2.0, 1.0])        # the noisy start, in another frame
    est = c2b.BAProblem.from_visibility(mc, mp, d["row_ptr"], d["pt_idx"], d["uv"])
    est.write(str(tmp / "est.bbal"))
    truth.write(str(tmp / "ref.bbal"))
    return entry.build_cli(), c2b, tmp


def run(cli, *args):
    r = subprocess.run([cli] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1                                     # ONE JSON line
    return json.loads(lines[0])


@pytest.mark.parametrize("flags", ((), ("--on", "both"), ("--on", "points", "--no-scale"), ("--on", "cameras", "--max-dist", "0.05", "--rounds", "2")))
def test_compare_prints_the_python_calls_numbers(setup, flags):
    cli, c2b, tmp = setup
    got = run(cli, "compare", tmp / "est.bbal", tmp / "ref.bbal", *flags)
    est, ref = c2b.BAProblem.from_file(str(tmp / "est.bbal")), c2b.BAProblem.from_file(str(tmp / "ref.bbal"))
    kw = dict(on=flags[flags.index("--on") + 1] if "--on" in flags else "cameras", scale="--no-scale" not in flags)
    if "--max-dist" in flags:
        kw.update(max_dist=0.05, rounds=2)
    want = est.align(ref, **kw)
    assert got["status"] == want["status"] == "ok" and got["rounds"] == want["rounds"]
    assert got["scale"] == want["scale"] and np.array_equal(np.array(got["rotation"]), want["rotation"]) and np.array_equal(np.array(got["translation"]), want["translation"])
    for kind in ("cameras", "points"):
        for k in ("n", "rmse", "mean", "max", "argmax"):
            assert got[kind][k] == want[kind][k], (kind, k)
    assert got["camera_rotations_deg"]["rmse"] == want["cameras"]["rot_rmse_deg"] and got["camera_rotations_deg"]["argmax"] == want["cameras"]["rot_argmax"]
    assert got["camera_rotations_deg"]["max"] == want["cameras"]["rot_max_deg"] and got["camera_rotations_deg"]["mean"] == want["cameras"]["rot_mean_deg"]
    if "--no-scale" in flags:
        assert got["scale"] == 1.0


def test_apply_writes_the_estimate_in_the_references_frame(setup):
    cli, c2b, tmp = setup
    first = run(cli, "compare", tmp / "est.bbal", tmp / "ref.bbal", "--on", "both", "--apply", tmp / "moved.bbal")
    again = run(cli, "compare", tmp / "moved.bbal", tmp / "ref.bbal", "--on", "both")
    est, ref = c2b.BAProblem.from_file(str(tmp / "moved.bbal")), c2b.BAProblem.from_file(str(tmp / "ref.bbal"))
    sel = (np.concatenate([est._camera_centers(), est.points()]), np.concatenate([ref._camera_centers(), ref.points()]))
    st, s, R, t, sig, eps = A.fit(*sel)
    m = A.moments(*sel)
    k = m["n"]
    cov = (m["sxy"] / k).astype(np.float64)
    d_sigma = float(np.sqrt((((k + 8) * U * m["abs_sxy"] / k) ** 2).sum())) + 64 * U * float(np.sqrt((cov * cov).sum()))
    dR, ds, dt = A.fit_bounds(m, sig, eps, s, d_sigma, (k + 8) * U)
    # the moved file's best similarity onto REF is the identity up to the rounding of the moved data: 8u (s |x| + |t|) per entity
    # (the transform's own bound; the .bbal holds to_vec of the cameras, another 64u of the centre), over the cloud's spread
    size = float(np.abs(sel[1]).max()) * np.sqrt(3.0)
    eps_d, spread = 72 * U * 2 * size, float(np.sqrt(sig[1] / s))
    assert again["status"] == "ok"
    assert abs(again["scale"] - 1.0) <= 4 * eps_d / spread + ds
    assert np.sqrt(((np.array(again["rotation"]) - np.eye(3)) ** 2).sum()) <= 4 * eps_d / spread + dR
    assert np.linalg.norm(again["translation"]) <= 4 * eps_d * (1 + float(np.linalg.norm(m["mean_x"].astype(np.float64))) / spread) + dt
    for kind in ("cameras", "points"):                        # the errors that remain are the first comparison's
        assert abs(again[kind]["rmse"] - first[kind]["rmse"]) <= 1e-9 * first[kind]["rmse"] + 4 * eps_d
