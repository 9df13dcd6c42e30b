"""`noise` has two single-GPU routes over one perturbation chain: the resident route (file decoded, noised and encoded on
the device) and, with C2B_HOST_IO=1, the host-array route (file read and written by the host, the problem uploaded in
between).  Same flags, same seed => the same file, byte for byte, and the same report lines, for .bbal and for .bal."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

FLAGS = ["--rotation-std", "0.01", "--translation-std", "0.02", "--point-std", "0.03", "--observation-std", "0.004",
         "--drift-strength", "0.001", "--drift-angle", "0.002", "--drift-std", "0.1", "--sin-strength", "0.05",
         "--sin-frequency", "2", "--seed", "5"]


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as entry
    return entry.build_cli()


def _run(cli, *args, **env):
    return subprocess.run([cli] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))


def _report(r):
    return [ln for ln in r.stdout.splitlines() if ln.startswith(("Initial error", "BA Problem", "Final error"))]


@pytest.mark.parametrize("ext", [".bbal", ".bal"])
def test_cli_noise_resident_and_host_routes_write_the_same_bytes(cli, tmp_path, ext):
    src = tmp_path / ("g" + ext)
    r = _run(cli, "synthetic", src, "--blocks", "3")
    assert r.returncode == 0, r.stderr
    resident, host = tmp_path / ("resident" + ext), tmp_path / ("host" + ext)
    ra = _run(cli, "noise", src, resident, *FLAGS)
    rb = _run(cli, "noise", src, host, *FLAGS, C2B_HOST_IO="1")
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr, rb.stderr)
    assert len(_report(ra)) == 3 and _report(ra) == _report(rb)
    assert _report(ra)[2] != "Final error: 0.00e0 (L1) 0.00e0 (L2)"                        # the noise really happened
    a, b = resident.read_bytes(), host.read_bytes()
    assert len(a) > 1000 and a != src.read_bytes()
    assert a == b
