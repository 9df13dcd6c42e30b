"""f32 extension (BASELINE.json configs[4]: "noise.rs drift+rotation kernels, f32 path").  The reference has no
f32 compute path; the float kernels are judged ENTRY BY ENTRY against the long-double reference of
tests/_noiseref.py on the float-rounded state, inside the running bound of the float instantiations (u = 2^-24):
|dev - ref| <= C E + |ref| 2^-60 + FLOOR.  Until then one bound scaled by the largest entry of the whole array judged them
(4e-6 to 2e-5 times max |value|), which hides a wrong small entry; the per-entry tolerance is at least as tight as that
bound on every entry (asserted here on the device's record, and in tests/test_noiseref.py on the CPU).  The kernels are
handed the record stats_f32 computed, so that record is itself held to the reference, slot by slot
(test_conversion_and_stats_f32).  More shapes and the edge cases: tests/test_gpu_noise_reference.py."""
import numpy as np
import pytest

import _noiseref as N
import oracle as O
from _problems import grid_cameras_points

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build()
    import torch
    import city2ba_amd
    from city2ba_amd import device as D
    assert city2ba_amd.device_count() > 0
    dev = torch.device("cuda", 0)
    cams, pts = grid_cameras_points(3, cpb=10, ppb=20, L=5.0)
    cam15 = torch.from_numpy(cams).to(dev)
    pts4 = D.points_pad(torch.from_numpy(pts).to(dev))
    ws = D.workspace(0, dev)
    return dict(torch=torch, D=D, dev=dev, cams=cams, pts=pts, cam15=cam15, pts4=pts4, ws=ws)


def _f32_state(env):
    D = env["D"]
    return D.to_f32(env["cam15"]), D.to_f32(env["pts4"])


def _back(env, c32, p32):
    D = env["D"]
    return D.to_f64(c32).cpu().numpy(), D.to_f64(p32).cpu().numpy()[:, :3]


def _judge(env, kind, st, got_c, got_p):
    """got_* = the float kernel's cameras / points (as f64), st = the record it was given; parameters and the earlier
    global bounds: N.F32_FILE_RUNS"""
    _, prm, old_c, old_p = next(r for r in N.F32_FILE_RUNS if r[0] == kind)
    c32, p32 = env["cams"].astype(np.float32).astype(np.float64), env["pts"].astype(np.float32).astype(np.float64)
    r = N.evaluate(kind, c32, p32, st.cpu().numpy(), prm, u=N.U32)
    tol_c, tol_p = N.tolerance(r["Ec"][:, :12], r["ref_c"][:, :12]), N.tolerance(r["Ep"], r["ref_p"])
    bc, bp = N.f32_old_bounds(r, old_c, old_p)
    assert bc is None or np.all(tol_c <= bc), (float(tol_c.max()), bc)      # no entry is judged more loosely than before
    assert np.all(tol_p <= bp), (float(tol_p.max()), bp)
    msgs = [N.report(got_c[:, :12], r["ref_c"][:, :12], r["Ec"][:, :12], kind + " cameras"), N.report(got_p, r["ref_p"], r["Ep"], kind + " points")]
    assert not any(msgs), "\n".join(m for m in msgs if m)
    assert np.array_equal(got_c[:, 12:15], c32[:, 12:15])                             # intrinsics untouched
    return prm


def test_conversion_and_stats_f32(env):
    D = env["D"]
    c32, p32 = _f32_state(env)
    c_back, p_back = _back(env, c32, p32)
    assert np.array_equal(c_back, env["cams"].astype(np.float32).astype(np.float64))
    assert np.array_equal(p_back, env["pts"].astype(np.float32).astype(np.float64))
    st = D.stats_f32(c32, p32, env["ws"]).cpu().numpy()
    assert np.allclose(st[0:3], O.mean(env["cams"], env["pts"]), rtol=1e-6, atol=1e-6)
    assert np.allclose(st[3:6], O.std(env["cams"], env["pts"]), rtol=1e-6)
    mn, mx = O.extent(env["cams"], env["pts"])
    assert np.allclose(st[6:9], mn, atol=1e-6) and np.allclose(st[9:12], mx, atol=1e-5)
    _, idx = O.drift_origin(env["cams"], env["pts"])
    assert int(st[18]) == idx
    # every slot against the long-double record of the float state: stats_f32 takes the centres in float (cm_center<float>: within
    # their u = 2^-24 bound of -R^T t) and accumulates in double at the device's depth
    c64, p64 = c_back, p_back
    cen, e_cen = N.device_centers(c64, u=N.U32)
    ent = np.concatenate([cen.astype(np.float64), p64])
    ref = N.statistics(c64, p64)
    E = N.stats_bound(ent, N.device_depth(len(ent)), e_ent=e_cen)
    msg = N.report(st, ref, E, "stats_f32")
    assert not msg, msg
    i = int(ref[18])
    assert int(st[18]) == i
    if i >= len(c64):                                         # the origin is a point: a selection of an input, exact; so are extremes
        assert np.array_equal(st[15:18], p64[i - len(c64)])   # that points hold
    for k in range(3):
        if p64[:, k].min() < (cen[:, k] - e_cen[:, k]).min():
            assert st[6 + k] == p64[:, k].min()
        if p64[:, k].max() > (cen[:, k] + e_cen[:, k]).max():
            assert st[9 + k] == p64[:, k].max()
    assert np.array_equal(st[12:15], st[9:12] - st[6:9])      # dimensions: THE difference of the extremes


def test_add_drift_f32_tracks_f64_oracle(env):
    D = env["D"]
    c32, p32 = _f32_state(env)
    st = D.stats_f32(c32, p32, env["ws"])
    d = np.array([0.3, -0.5, 0.8])
    D.add_drift_f32(c32, p32, st, 1e-3, 2e-3, 0.2, d, seed=42)
    got_c, got_p = _back(env, c32, p32)
    want_c, want_p = O.add_drift(env["cams"], env["pts"], 1e-3, 2e-3, 0.2, d, seed=42)
    _judge(env, "drift", st, got_c, got_p)
    # and it really moved things (not a no-op)
    assert np.max(np.abs(want_p - env["pts"])) > 1e-3


def test_add_noise_entities_f32_tracks_f64_oracle(env):
    D = env["D"]
    c32, p32 = _f32_state(env)
    st = D.stats_f32(c32, p32, env["ws"])
    D.add_noise_entities_f32(c32, p32, st, 0.1, 0.1, 0.1, seed=99)
    got_c, got_p = _back(env, c32, p32)
    want_c, want_p, _ = O.add_noise(env["cams"], env["pts"], np.zeros((0, 2)), 0.1, 0.1, 0.1, 0.0, seed=99)
    _judge(env, "noise", st, got_c, got_p)
    R = got_c[:, :9].reshape(-1, 3, 3)
    assert np.max(np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3))) < 1e-5       # still rotations


def test_normalized_drift_and_sin_f32(env):
    D = env["D"]
    c32, p32 = _f32_state(env)
    st = D.stats_f32(c32, p32, env["ws"])
    D.add_drift_normalized_f32(c32, p32, st, 0.01, 0.01, 0.1, seed=7)
    got_c, got_p = _back(env, c32, p32)
    want_c, want_p = O.add_drift_normalized(env["cams"], env["pts"], 0.01, 0.01, 0.1, seed=7)
    _judge(env, "drift_normalized", st, got_c, got_p)
    c32, p32 = _f32_state(env)
    D.add_sin_noise_f32(c32, p32, st, [1.0, 1.0, 0.0], [0.0, 1.0, 0.0], 1.0, 2.0)
    got_c, got_p = _back(env, c32, p32)
    want_c, want_p = O.add_sin_noise(env["cams"], env["pts"], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0], 1.0, 2.0)
    _judge(env, "sin", st, got_c, got_p)
