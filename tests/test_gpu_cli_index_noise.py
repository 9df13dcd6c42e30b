"""`city2ba noise ... --index-noise device` on the GPU: the file it writes is, byte for byte, the file Python writes after the
same chain of BAProblem methods in the reference's order (src/bin/city2ba.rs:288-303, :341) with the seeds s+2 ... s+5; without
the flag the output is the host route's, byte for byte; and the flag is refused beside --gpus."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

SEED = 11
ARITH = ["--rotation-std", "0.01", "--translation-std", "0.02", "--point-std", "0.03", "--observation-std", "0.004",
         "--drift-strength", "0.001", "--drift-angle", "0.002", "--drift-std", "0.1"]
INDEX = ["--drop-features", "0.8", "--split-landmarks", "0.1", "--join-landmarks", "0.05", "--mismatch-chance", "0.05"]


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as entry
    entry.build()
    return entry.build_cli()


@pytest.fixture(scope="module")
def src(cli, tmp_path_factory):
    path = tmp_path_factory.mktemp("index_noise") / "g.bbal"
    r = _run(cli, "synthetic", path, "--blocks", "3")
    assert r.returncode == 0, r.stderr
    return path


def _run(cli, *args, **env):
    return subprocess.run([cli] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))


def _report(r):
    return [ln for ln in r.stdout.splitlines() if ln.startswith(("Initial error", "BA Problem", "Final error"))]


def test_cli_device_route_writes_what_the_python_chain_writes(cli, src, tmp_path):
    import city2ba_amd as c2b
    from city2ba_amd import noise
    out_cli, out_py = tmp_path / "cli.bbal", tmp_path / "py.bbal"
    r = _run(cli, "noise", src, out_cli, *ARITH, *INDEX, "--seed", SEED, "--index-noise", "device", C2B_TIMING="1")
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert len(_report(r)) == 3, r.stdout
    assert "drop_features + cull (device)" in r.stderr and "download" not in r.stderr          # the phases of the resident route

    ba = c2b.BAProblem.from_file(str(src))
    assert ba.drop_features(0.8, seed=SEED + 2) > 0
    ba.cull()
    assert ba.join_landmarks(0.1, seed=SEED + 3) > 0         # the SPLIT fraction: the reference's quirk (src/bin/city2ba.rs:296)
    ba.cull()
    assert ba.split_landmarks(0.1, seed=SEED + 4) > 0
    ba.cull()
    noise.add_drift_normalized(ba, 0.001, 0.002, 0.1, seed=SEED)
    noise.add_noise(ba, 0.02, 0.01, 0.03, 0.004, seed=SEED + 1)
    assert ba.add_incorrect_correspondences(0.05, seed=SEED + 5) > 0
    l1, l2 = ba.total_reprojection_errors_l1_l2()
    sizes = (ba.num_cameras(), ba.num_points(), ba.num_observations())
    ba.write(str(out_py))
    ba.close()
    assert out_cli.read_bytes() == out_py.read_bytes()
    assert out_cli.read_bytes() != src.read_bytes()
    assert all(str(n) in _report(r)[1] for n in sizes), (_report(r), sizes)
    assert _report(r)[2] == "Final error: %s (L1) %s (L2)" % tuple(_rust_e(v) for v in (l1, l2)), (_report(r), l1, l2)


def _rust_e(v):
    """Rust's {:.2e}"""
    m, e = ("%.2e" % v).split("e")
    return "%se%d" % (m, int(e))


def test_cli_default_is_the_host_route_byte_for_byte(cli, src, tmp_path):
    plain, host, dev = tmp_path / "plain.bbal", tmp_path / "host.bbal", tmp_path / "dev.bbal"
    ra = _run(cli, "noise", src, plain, *ARITH, *INDEX, "--seed", SEED)
    rb = _run(cli, "noise", src, host, *ARITH, *INDEX, "--seed", SEED, "--index-noise", "host")
    rc = _run(cli, "noise", src, dev, *ARITH, *INDEX, "--seed", SEED, "--index-noise", "device")
    assert ra.returncode == 0 and rb.returncode == 0 and rc.returncode == 0, (ra.stderr, rb.stderr, rc.stderr)
    assert plain.read_bytes() == host.read_bytes() and _report(ra) == _report(rb) and len(_report(ra)) == 3
    assert dev.read_bytes() != host.read_bytes()             # another draw scheme
    assert _report(rc)[0] == _report(ra)[0]                  # the same input: the same initial error


def test_cli_device_route_refuses_sharding(cli, src, tmp_path):
    out = tmp_path / "o.bbal"
    for extra in (("--gpus", "1"), ("--devices", "0")):
        r = _run(cli, "noise", src, out, *INDEX, "--index-noise", "device", *extra)
        assert r.returncode != 0 and "--index-noise device runs on one GPU" in r.stderr, r.stderr
    assert not out.exists()
