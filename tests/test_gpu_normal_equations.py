"""The Gauss-Newton diagonal blocks on the device: c2b_problem_normal_equations (BAProblem.normal_equations) and its
Level-0 passes (c2b_normal_transpose, c2b_normal_cameras_rows, c2b_normal_points_rows).

U = sum Jc^T Jc, gc = sum Jc^T r per camera, V = sum Jp^T Jp, gp = sum Jp^T r per point, from the device's own
per-observation Jacobian (c2b_problem_residual_jacobian): every entry within (k + 4) 2^-53 S_ab of the longdouble sum
(tests/_normref.py: a bound that holds for any summation order), and the exact properties the kernels promise --
symmetry, zeros, run-to-run bits, shard rows equal to the whole problem's, a fresh transpose after the list changes --
plus what a solver needs: one undamped Gauss-Newton step from them cuts the error of a perturbed exact problem 100x."""
import argparse
import ctypes as C

import numpy as np
import pytest

import _normref as R
import oracle as O
from _problems import mixed_k2_cameras, random_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build()
    import torch
    import city2ba_amd
    from city2ba_amd import device as D
    assert city2ba_amd.device_count() > 0
    return dict(torch=torch, D=D, dev=torch.device("cuda", 0))


def _np(t):
    return t.cpu().numpy()


def _cam_of(row_ptr):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))


def _reference(ba):
    r, Jc, Jp = ba.residual_jacobian()
    return R.blocks(r, Jc, Jp, _cam_of(ba.row_ptr), ba.pt_idx.astype(np.int64), ba.num_cameras(), ba.num_points())


def _check_problem(ba, kind):
    U, gc, V, gp, s = ba.normal_equations()
    dev = tuple(_np(a) for a in (U, gc, V, gp))
    ref = _reference(ba)
    R.check(dev, ref, kind)
    e2 = ba.total_reprojection_error(2.0) ** 2
    assert abs(s - e2) <= 1e-12 * e2, (kind, s, e2)
    return dev, ref


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. transpose -----------------------------------------------------------------------------------------------
def _list(kind, seed):
    """(row_ptr, pt_idx, n_pts) of a camera-major list with the shape `kind`"""
    rng = np.random.default_rng(seed)
    if kind == "ragged":
        counts = rng.integers(0, 40, 150)
        n_pts = 900
    elif kind == "empties":
        counts = rng.integers(0, 12, 300) * (rng.random(300) < 0.5)
        n_pts = 2000                                             # most points unobserved
    elif kind == "singles":
        counts = np.ones(517, dtype=np.int64)                    # n_obs not a multiple of 64
        n_pts = 517
    else:                                                        # "crowded": point 7 is seen by 300 cameras
        counts = rng.integers(1, 9, 300)
        n_pts = 400
    counts = np.asarray(counts, dtype=np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(row_ptr[-1])
    if kind == "singles":
        pt_idx = rng.permutation(n)                              # every point exactly one observation
    else:
        pt_idx = rng.integers(0, n_pts, n)
        if kind == "ragged":
            pt_idx[rng.random(n) < 0.2] = 3                      # a point seen many times, unsorted within lists
        if kind == "crowded":
            pt_idx[row_ptr[:-1]] = 7
    return row_ptr, pt_idx.astype(np.int64), n_pts


@pytest.mark.parametrize("kind", ["ragged", "empties", "singles", "crowded"])
def test_transpose_is_the_stable_argsort(env, kind):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    row_ptr, pt_idx, n_pts = _list(kind, seed={"ragged": 1, "empties": 2, "singles": 3, "crowded": 4}[kind])
    n = len(pt_idx)
    if kind == "crowded":
        assert np.sum(pt_idx == 7) > 64
    rows = D.Rows(torch.from_numpy(row_ptr).to(dev), n)
    pr = D.PointRows(rows, torch.from_numpy(pt_idx.astype(np.int32)).to(dev), n_pts)
    torch.cuda.synchronize()
    want = np.argsort(pt_idx, kind="stable")
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(pt_idx, minlength=n_pts))])
    assert np.array_equal(_np(pr.pt_row_ptr), want_ptr)
    assert np.array_equal(_np(pr.obs_of).astype(np.int64), want)
    assert np.array_equal(_np(pr.cam_of).astype(np.int64), _cam_of(row_ptr)[want])


# ---- 2. accuracy ------------------------------------------------------------------------------------------------
def test_accuracy_bal_mode_then_state_mode_after_drift(env):
    import city2ba_amd as c2b
    from city2ba_amd import noise as N
    P = random_problem(120, 3000, 25, seed=11, noise=1e-3, empty_every=17)
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    _check_problem(ba, "bal")
    N.add_drift(ba, 0.05, 0.01, 0.01, [1.0, 0.5, 0.0], seed=4)   # leaves bal mode
    _check_problem(ba, "state")
    ba.close()


@pytest.mark.parametrize("pattern", ["half", "signs"])
def test_accuracy_with_mixed_k2(env, pattern):
    import city2ba_amd as c2b
    P = random_problem(90, 2500, 30, seed=23)
    cams = mixed_k2_cameras(P["cams15"], pattern, seed=5)
    uv = O.project_observations(cams, P["pts"], P["row_ptr"], P["pt_idx"])
    uv = uv + np.random.default_rng(8).normal(scale=1e-3, size=uv.shape)
    ba = c2b.BAProblem.from_visibility(cams, P["pts"], P["row_ptr"], P["pt_idx"], uv, device=0)
    _check_problem(ba, "k2 " + pattern)
    ba.close()


def _grid(cull):
    from city2ba_amd import synthetic as S
    g = S.synthetic_grid(3, 20, 3, 5.0, 1.0, 1.0, 1.0, 10.0, False, cull=False)      # un-culled: empty cameras
    if cull:
        g.cull()
    return g


def test_accuracy_on_a_grid_with_shared_points(env):
    import city2ba_amd as c2b
    g = _grid(cull=False)
    uv = g.observations() + np.random.default_rng(3).normal(scale=1e-2, size=(g.num_observations(), 2))
    ba = c2b.BAProblem.from_visibility(g.cameras(), g.points(), g.row_ptr.copy(), g.pt_idx.copy(), uv)
    g.close()
    (U, gc, V, gp), ref = _check_problem(ba, "grid")
    assert (ref["kp"] > 1).sum() > 100 and (ref["kc"] == 0).any()
    ba.close()


# ---- 3. exact properties ----------------------------------------------------------------------------------------
def test_symmetry_zeros_repeatability_and_level0_bits(env):
    import city2ba_amd as c2b
    torch, D, dev = env["torch"], env["D"], env["dev"]
    P = random_problem(150, 4000, 21, seed=31, noise=1e-3, empty_every=9)
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    U, gc, V, gp, s = ba.normal_equations()
    for a in (U, gc, V, gp):
        assert a.device == dev and a.dtype == torch.float64 and a.is_contiguous()
    Un, Vn = _np(U), _np(V)
    assert _same_bits(Un, Un.transpose(0, 2, 1)) and _same_bits(Vn, Vn.transpose(0, 2, 1))
    kc = np.diff(P["row_ptr"].astype(np.int64))
    kp = np.bincount(P["pt_idx"].astype(np.int64), minlength=len(P["pts"]))
    assert (kc == 0).any() and (kp == 0).any()
    assert _same_bits(Un[kc == 0], np.zeros((int((kc == 0).sum()), 9, 9))) and not _np(gc)[kc == 0].any()
    assert _same_bits(Vn[kp == 0], np.zeros((int((kp == 0).sum()), 3, 3))) and not _np(gp)[kp == 0].any()
    assert Un[kc > 0].any(axis=(1, 2)).all() and Vn[kp > 0].any(axis=(1, 2)).all()

    out = tuple(torch.full_like(a, float("nan")) for a in (U, gc, V, gp))
    U2, gc2, V2, gp2, s2 = ba.normal_equations(out=out)
    assert all(x is y for x, y in zip((U2, gc2, V2, gp2), out))
    assert all(torch.equal(a, b) for a, b in zip((U, gc, V, gp), out)) and s2 == s

    # Level 0 over the same inputs: the same bits
    camblk = D.cameras_prepare_bal(torch.from_numpy(P["bal9"]).to(dev))
    pts4 = D.points_pad(torch.from_numpy(P["pts"]).to(dev))
    rows = D.Rows(torch.from_numpy(P["row_ptr"].astype(np.int64)).to(dev))
    pi = torch.from_numpy(P["pt_idx"].astype(np.int32)).to(dev)
    uv = torch.from_numpy(P["uv"]).to(dev)
    ws = D.workspace(rows.n_obs, dev)
    s0 = torch.zeros(1, dtype=torch.float64, device=dev)
    U0, gc0 = torch.empty_like(U), torch.empty_like(gc)
    V0, gp0 = torch.empty_like(V), torch.empty_like(gp)
    D.normal_cameras_rows(camblk, pts4, rows, pi, uv, U0, gc0, ws, s0)
    D.normal_points_rows(camblk, pts4, D.PointRows(rows, pi, len(P["pts"])), uv, V0, gp0)
    torch.cuda.synchronize()
    assert torch.equal(U0, U) and torch.equal(gc0, gc) and torch.equal(V0, V) and torch.equal(gp0, gp)
    assert s0.item() == s
    # one pass alone: the other pair untouched
    Vn2 = torch.full_like(V, float("nan"))
    ba.normal_equations(out=(U0, gc0, None, None))
    ba.normal_equations(out=(None, None, Vn2, gp0))
    assert torch.equal(U0, U) and torch.equal(Vn2, V)
    ba.close()


def test_shards_give_the_whole_problems_camera_rows(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    P = random_problem(200, 5000, 20, seed=47, noise=1e-3, empty_every=13)
    cams, pts, rp, pi, uv = P["cams15"], P["pts"], P["row_ptr"].astype(np.int64), P["pt_idx"], P["uv"]
    whole = c2b.BAProblem.from_visibility(cams, pts, P["row_ptr"], pi, uv, device=0)
    U, gc, V, gp, s = (x if isinstance(x, float) else _np(x) for x in whole.normal_equations())
    ref = _reference(whole)
    Vsum, gpsum = np.zeros_like(V), np.zeros_like(gp)
    for lo, hi in ((0, 77), (77, 200)):
        o0, o1 = int(rp[lo]), int(rp[hi])
        sh = c2b.BAProblem.from_visibility(cams[lo:hi], pts, (rp[lo:hi + 1] - o0).astype(np.uint64), pi[o0:o1], uv[o0:o1], device=0)
        L.check(L.lib().c2b_problem_set_shard(sh._h, lo, 200, o0))
        Ua, gca, Va, gpa, _ = sh.normal_equations()
        assert _same_bits(_np(Ua), U[lo:hi]) and _same_bits(_np(gca), gc[lo:hi])
        Vsum += _np(Va)
        gpsum += _np(gpa)
        sh.close()
    for name, a, key, S in (("V", Vsum, "V", "SV"), ("gp", gpsum, "gp", "Sgp")):
        assert R.excess(a, ref[key], ref[S], ref["kp"]) <= 1.0, name
    whole.close()


# ---- 4. cache invalidation --------------------------------------------------------------------------------------
def test_transpose_is_rebuilt_after_cull_and_upload(env):
    import city2ba_amd as c2b
    g = _grid(cull=False)
    uv = g.observations() + np.random.default_rng(5).normal(scale=1e-2, size=(g.num_observations(), 2))
    ba = c2b.BAProblem.from_visibility(g.cameras(), g.points(), g.row_ptr.copy(), g.pt_idx.copy(), uv)
    g.close()

    def fresh_equal(ba):
        got = ba.normal_equations()
        f = c2b.BAProblem.from_visibility(ba.cameras(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations())
        want = f.normal_equations()
        f.close()
        assert all(_same_bits(_np(a), _np(b)) for a, b in zip(got[:4], want[:4]))
        assert got[4] == want[4]

    fresh_equal(ba)
    n0 = ba.num_observations()
    ba.cull()
    assert ba.num_observations() < n0
    fresh_equal(ba)
    P = random_problem(60, 1500, 15, seed=3, noise=1e-3)
    ba._upload(P["cams15"], False, P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])
    fresh_equal(ba)
    ba.close()


# ---- 5. what a solver needs ------------------------------------------------------------------------------------
def _solve(A, b):
    if np.linalg.cond(A) > 1e12:
        return np.linalg.lstsq(A, b, rcond=None)[0]
    return np.linalg.solve(A, b)


def test_one_gauss_newton_step_on_cameras_then_on_points(env):
    import city2ba_amd as c2b
    g = _grid(cull=True)
    bal9, pts, rp, pi = g.cameras_bal(), g.points(), g.row_ptr.copy(), g.pt_idx.copy()
    uv = g.project()                                                  # exact observations
    g.close()
    rng = np.random.default_rng(12)
    mk = lambda b9, X: c2b.BAProblem.from_bal(b9, X, rp, pi, uv, device=0)

    # cameras: w and t moved by ~1e-4, points fixed -> the cameras are independent
    b9 = bal9.copy()
    b9[:, :6] += rng.normal(scale=1e-4, size=(len(b9), 6))
    ba = mk(b9, pts)
    e0 = ba.total_reprojection_error(2.0)
    U, gc, _, _, _ = ba.normal_equations()
    U, gc = _np(U), _np(gc)
    delta = np.stack([_solve(U[c], -gc[c]) for c in range(len(b9))])
    ba.close()
    ba = mk(b9 + delta, pts)
    e1 = ba.total_reprojection_error(2.0)
    ba.close()
    assert e0 > 1e-6 and e1 <= e0 / 100.0, (e0, e1)

    # points with at least two observations, cameras fixed
    kp = np.bincount(pi.astype(np.int64), minlength=len(pts))
    moved = kp >= 2
    assert moved.sum() > 50
    X = pts.copy()
    X[moved] += rng.normal(scale=1e-4, size=(int(moved.sum()), 3))
    ba = mk(bal9, X)
    e0 = ba.total_reprojection_error(2.0)
    _, _, V, gp, _ = ba.normal_equations()
    V, gp = _np(V), _np(gp)
    X1 = X.copy()
    for p in np.nonzero(moved)[0]:
        X1[p] += _solve(V[p], -gp[p])
    ba.close()
    ba = mk(bal9, X1)
    e1 = ba.total_reprojection_error(2.0)
    ba.close()
    assert e0 > 1e-6 and e1 <= e0 / 100.0, (e0, e1)


# ---- 6. full size -----------------------------------------------------------------------------------------------
def test_full_size_sample_at_blocks_32(env):
    import bench
    torch, D, dev = env["torch"], env["D"], env["dev"]
    sh = bench.build_shard(argparse.Namespace(blocks=32), 0, 1, dev)
    n, rows, pts4, pi, uv, camblk = sh["n_obs"], sh["rows"], sh["pts4"], sh["pt_idx"], sh["uv"], sh["camblk"]
    assert n == 1_225_066
    n_cam, n_pts = rows.n_cam, pts4.shape[0]
    U = torch.empty((n_cam, 9, 9), dtype=torch.float64, device=dev)
    gc = torch.empty((n_cam, 9), dtype=torch.float64, device=dev)
    V = torch.empty((n_pts, 3, 3), dtype=torch.float64, device=dev)
    gp = torch.empty((n_pts, 3), dtype=torch.float64, device=dev)
    D.normal_cameras_rows(camblk, pts4, rows, pi, uv, U, gc)
    D.normal_points_rows(camblk, pts4, D.PointRows(rows, pi, n_pts), uv, V, gp)
    r = torch.empty((n, 2), dtype=torch.float64, device=dev)
    Jc = torch.empty((n, 18), dtype=torch.float64, device=dev)
    Jp = torch.empty((n, 6), dtype=torch.float64, device=dev)
    D.residual_jacobian_rows(camblk, pts4, rows, pi, uv, r, Jc, Jp)
    torch.cuda.synchronize()
    rp, pt = _np(rows.row_ptr), _np(pi).astype(np.int64)
    cam_of = _cam_of(rp)
    rng = np.random.default_rng(2024)
    cs = rng.choice(n_cam, 2000, replace=False)
    ps = rng.choice(np.unique(pt), 2000, replace=False)
    obs_c = np.concatenate([np.arange(rp[c], rp[c + 1]) for c in cs])
    obs_p = np.nonzero(np.isin(pt, ps))[0]
    local_c = np.repeat(np.arange(len(cs)), np.diff(rp)[cs])
    local_p = np.searchsorted(np.sort(ps), pt[obs_p])
    ps = np.sort(ps)
    take = lambda t, idx: _np(t[torch.from_numpy(idx).to(dev)])
    refc = R.blocks(take(r, obs_c), take(Jc, obs_c), take(Jp, obs_c), local_c, np.zeros(len(obs_c), dtype=np.int64), len(cs), 1)
    refp = R.blocks(take(r, obs_p), take(Jc, obs_p), take(Jp, obs_p), np.zeros(len(obs_p), dtype=np.int64), local_p, 1, len(ps))
    assert np.array_equal(cam_of[obs_c], np.repeat(cs, np.diff(rp)[cs]))
    for name, a, ref, key, S, k in (("U", _np(U)[cs], refc, "U", "SU", "kc"), ("gc", _np(gc)[cs], refc, "gc", "Sgc", "kc"),
                                    ("V", _np(V)[ps], refp, "V", "SV", "kp"), ("gp", _np(gp)[ps], refp, "gp", "Sgp", "kp")):
        assert R.excess(a, ref[key], ref[S], ref[k]) <= 1.0, name


# ---- 7. bad arguments ---------------------------------------------------------------------------------------------
def test_bad_arguments(env):
    import city2ba_amd as c2b
    from city2ba_amd import _lib as L
    torch, dev = env["torch"], env["dev"]
    lib = L.lib()
    P = random_problem(20, 300, 10, seed=1, noise=1e-3)
    ba = c2b.BAProblem.from_visibility(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    nc, npt = ba.num_cameras(), ba.num_points()
    U = torch.full((nc, 9, 9), float("nan"), dtype=torch.float64, device=dev)
    gc = torch.full((nc, 9), float("nan"), dtype=torch.float64, device=dev)
    V = torch.full((npt, 3, 3), float("nan"), dtype=torch.float64, device=dev)
    gp = torch.full((npt, 3), float("nan"), dtype=torch.float64, device=dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    s = C.c_double(-1.0)
    bad = [
        (None, p(U), p(gc), p(V), p(gp)),
        (ba._h, p(U), None, p(V), p(gp)),
        (ba._h, None, p(gc), None, None),
        (ba._h, p(U), p(gc), p(V), None),
        (ba._h, None, None, None, p(gp)),
        (ba._h, p(U, 4), p(gc), None, None),
        (ba._h, None, None, p(V), p(gp, 1)),
    ]
    for args in bad:
        assert lib.c2b_problem_normal_equations(*args, C.byref(s)) == L.ERR_INVALID_ARGUMENT, args
    assert lib.c2b_problem_normal_equations(ba._h, p(U), p(gc), p(V), p(gp), C.cast(C.c_void_p(8 * 1000 + 3), C.POINTER(C.c_double))) == L.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert s.value == -1.0 and all(bool(torch.isnan(t).all()) for t in (U, gc, V, gp))
    assert b"pairs" in lib.c2b_last_error() or b"misaligned" in lib.c2b_last_error()
    for out in ((U[:-1], gc, V, gp), (U, gc.float(), V, gp), (U, gc, V.cpu(), gp), (U, gc, V.transpose(1, 2), gp),
                (U, None, V, gp), (U, gc, V)):
        with pytest.raises(ValueError):
            ba.normal_equations(out=out)
    assert all(bool(torch.isnan(t).all()) for t in (U, gc, V, gp))
    # Level 0: a NULL output, misaligned temp
    D = env["D"]
    assert lib.c2b_normal_cameras_rows(None, None, None, 3, None, None, 0, None, None, None, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_normal_points_rows(None, None, 5, None, None, None, None, None, None, None) == L.ERR_INVALID_ARGUMENT
    rp = torch.from_numpy(P["row_ptr"].astype(np.int64)).to(dev)
    pi = torch.from_numpy(P["pt_idx"].astype(np.int32)).to(dev)
    tmp = torch.empty(4096, dtype=torch.float64, device=dev)
    ptr = torch.empty(npt + 1, dtype=torch.int64, device=dev)
    oo = torch.empty(len(P["pt_idx"]), dtype=torch.int32, device=dev)
    assert lib.c2b_normal_transpose(p(rp), nc, p(pi), len(P["pt_idx"]), npt, p(ptr), p(oo), p(oo), p(tmp, 8), None) == L.ERR_INVALID_ARGUMENT
    ba.close()
