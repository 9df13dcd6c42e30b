"""The device Levenberg-Marquardt step on a coupled, ragged, general-position problem (tests/_problems.py's dome_problem:
general rotations, mixed distortion, points shared between cameras, camera rows of length 0, 1, 15, 16, 17, ... 257 side
by side in one wave, a point row longer than a wave, (camera, point) pairs that repeat), against the longdouble
references of tests/_normref.py, _schurref.py, _precondref.py and _robustref.py built from the device's own Jacobian
(BAProblem.residual_jacobian), with the checkers of tests/_solvecheck.py that the other solver tests use.  What the
problem and the references must provide is asserted on the CPU by tests/test_coupled_problem.py; the compared iterates
are _solvecheck.DOME_KS, and at each of them the reference's own bound is again held under _solvecheck.DOME_CAP here.
Worst |err| / bound seen on the MI355X (the PCGREF / SJREF lines this prints): DESIGN 4.6."""
import numpy as np
import pytest

import _normref as NR
import _precondref as PR
import _robustref as B
import _schurref as R
import _solvecheck as SC
from _problems import DOME_CROWDED, dome_problem
from test_gpu_robust_loss import _WEIGHT_OPS
from test_gpu_schur_jacobi import _device_blocks
from test_gpu_schur_step import EPS, _bits, _kappa, _level0, _make, _np, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
MODES = ["bal", "state"]
KINDS = ["block_jacobi", "schur_jacobi"]
_cache = {}


def _dome(mode="bal", dup=True):
    key = ("dome", mode, dup)
    if key not in _cache:
        _cache[key] = dome_problem(dup=dup, state=mode == "state")
    return _cache[key]


def _load(P, uv=None):
    import city2ba_amd as c2b
    uv = P["uv"] if uv is None else uv
    if P["bal"]:
        return c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], uv, device=0)
    return c2b.BAProblem.from_visibility(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], uv, device=0)


def _lin(ba, dtype=R.LD, loss=None, mask=None):
    """the reference problem of the device's own linearisation"""
    r, Jc, Jp = ba.residual_jacobian()
    return SC.linearisation(r, Jc, Jp, ba.row_ptr, ba.pt_idx, ba.num_cameras(), ba.num_points(), dtype, loss, mask)


def _reference(key, ba, lam, ks, kind, loss=None, mask=None):
    """(P, pcg reference) of one case, computed once per module and left unchanged"""
    key = ("ref",) + key
    if key not in _cache:
        P = _lin(ba, loss=loss, mask=mask)
        ref = PR.pcg(P, lam, max(ks), 0.0, kind=kind, runs=8)
        cap = SC.cap_excess(ref, ks)
        assert cap <= 1.0, (key, "the reference's own bound exceeds 1e-6 of an iterate", cap)
        _cache[key] = (P, ref)
    return _cache[key]


def _rows_check(got, want, scale, what, tag, kc):
    """err <= 1e-12 |scale| in norm and row by row (camera by camera / point by point); the worst row is named"""
    err = (np.asarray(got).astype(R.LD) - want).astype(np.float64)
    total = float(np.linalg.norm(err)) / float(np.linalg.norm(scale.astype(np.float64)))
    ov = SC.rows_over(err, scale, 1e-12)
    w = int(ov.argmax())
    print("COUPLED operator %s %s: |err| / |scale| %.3g; worst row %d (length %d) %.3g x its 1e-12 scale" % (tag, what, total, w, kc[w], ov[w]))
    assert total <= 1e-12, (tag, what, total)
    assert ov[w] <= 1.0, (tag, what, "row", w, "length", int(kc[w]), float(ov[w]))


def _operator(env, ba, bal, ref, tag, loss=None):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    nc, npt = ba.num_cameras(), ba.num_points()
    U, gc, V, gp, _ = ba.normal_equations()
    camblk, pts4, rows, prows, pi, uv = _level0(env, ba, bal)
    f64 = dict(dtype=torch.float64, device=dev)
    t, y = torch.empty((npt, 3), **f64), torch.empty((nc, 9), **f64)
    kc = np.diff(ba.row_ptr.astype(np.int64))
    kp = np.bincount(ba.pt_idx.astype(np.int64), minlength=npt)
    rng = np.random.default_rng(7)
    for lam in (1e-2, 1.0):
        x = rng.normal(size=(nc, 9))
        xt = torch.from_numpy(x).to(dev)
        D.schur_points_rows(camblk, pts4, prows, uv, V, lam, xt, None, t, loss=loss)
        D.schur_cameras_rows(camblk, pts4, rows, pi, uv, U, lam, xt, t, y, loss=loss)
        _rows_check(_np(y), *ref.S_times(lam, x), "S x", "%s lam=%g" % (tag, lam), kc)
        D.schur_points_rows(camblk, pts4, prows, uv, V, lam, None, gp, t, loss=loss)
        D.schur_cameras_rows(camblk, pts4, rows, pi, uv, U, lam, None, t, y, loss=loss)
        _rows_check(-_np(gc) - _np(y), *ref.rhs(lam), "b", "%s lam=%g" % (tag, lam), kc)
        D.schur_points_rows(camblk, pts4, prows, uv, V, lam, xt, gp, t, loss=loss)
        _rows_check(-_np(t), *ref.back_substitute(lam, x), "dp", "%s lam=%g" % (tag, lam), kp)


# ---- 1. normal equations ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_normal_equations(env, mode):
    ba = _load(_dome(mode))
    nc, npt = ba.num_cameras(), ba.num_points()
    U, gc, V, gp, s = ba.normal_equations()
    dev = tuple(_np(a) for a in (U, gc, V, gp))
    r, Jc, Jp = ba.residual_jacobian()
    ref = NR.blocks(r, Jc, Jp, SC.cam_of(ba.row_ptr), ba.pt_idx.astype(np.int64), nc, npt)
    print("COUPLED blocks %s: |err| / bound %s" % (mode, {k: "%.3g" % NR.excess(a, ref[k], ref["S" + k], ref[n])
                                                       for a, k, n in zip(dev, ("U", "gc", "V", "gp"), ("kc", "kc", "kp", "kp"))}))
    NR.check(dev, ref, "dome " + mode)
    e2 = ba.total_reprojection_error(2.0) ** 2
    assert abs(s - e2) <= 1e-12 * e2 and abs(s - float(ref["sum_sq"])) <= 1e-12 * e2, (s, e2, float(ref["sum_sq"]))
    Un, gcn, Vn, gpn = dev
    kc, kp = ref["kc"], ref["kp"]
    assert (kc == 0).sum() == 1 and (kp == 0).sum() == 20 and kp.max() > 64
    assert not Un[kc == 0].any() and not gcn[kc == 0].any() and not Vn[kp == 0].any() and not gpn[kp == 0].any()
    assert _bits(Un[kc == 0], np.zeros((1, 9, 9))) and _bits(Vn[kp == 0], np.zeros((20, 3, 3)))      # +0, not -0
    assert _bits(Un, Un.transpose(0, 2, 1)) and _bits(Vn, Vn.transpose(0, 2, 1))
    assert Un[kc > 0].any(axis=(1, 2)).all() and Vn[kp > 0].any(axis=(1, 2)).all()
    ba.close()


# ---- 2. operator, right-hand side, back-substitution --------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_operator_rhs_and_back_substitution(env, mode):
    P = _dome(mode)
    ba = _load(P)
    _operator(env, ba, P["bal"], _lin(ba), "dome " + mode)
    ba.close()


# ---- 3. Schur-Jacobi blocks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dup", [True, False], ids=["dup", "nodup"])
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_schur_jacobi_blocks(env, lam, dup):
    P = _dome("bal", dup)
    ba = _load(P)
    Q = _lin(ba)
    assert PR.has_duplicate_pairs(Q) == dup
    M = _device_blocks(env, ba, True, lam)
    ov = SC.check_blocks(M, Q, lam, "dome %s" % ("dup" if dup else "nodup"), runs=8)
    kc = np.diff(ba.row_ptr.astype(np.int64))
    print("COUPLED blocks worst camera %d (length %d)" % (int(ov.argmax()), kc[int(ov.argmax())]))
    assert _bits(M[kc == 0], np.diag(np.full(9, lam * 1e-6))[None])          # an empty camera: the damping's diagonal
    if not dup:
        # no pair repeats: the blocks are S's diagonal blocks, to the reference's bound plus what its two forms differ by
        Mref, bound, _ = PR.blocks_bound(Q, lam, runs=8)
        Dg, _ = PR.schur_diag_blocks(Q, lam)
        gap = np.linalg.norm((Mref - Dg).astype(np.float64), axis=(1, 2))
        err = np.linalg.norm(M - Dg.astype(np.float64), axis=(1, 2))
        assert (err <= bound + gap).all(), int((err - bound - gap).argmax())
    ba.close()


# ---- 4. PCG iterates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("kind", KINDS)
def test_pcg_iterates_follow_the_reference(env, kind, lam, mode):
    ba = _load(_dome(mode))
    ba.set_preconditioner(kind)
    ks = SC.DOME_KS[(kind, lam)]
    Q, ref = _reference((mode, kind, lam), ba, lam, ks, kind)
    SC.check_iterates(ba, Q, ref, lam, ks, tag="coupled %s %s" % (kind, mode), label="PCGREF")
    assert ba.preconditioner_fallbacks() == 0
    ba.close()


# ---- 5. stopping ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_stopping_iteration_is_exact(env, kind):
    lam = 1e-4
    ba = _load(_dome("bal"))
    ba.set_preconditioner(kind)
    _, ref = _reference(("bal", kind, lam), ba, lam, SC.DOME_KS[(kind, lam)], kind)
    tols = SC.crossing_tols(ref, 4)
    assert len(tols) >= 3, ref["rel"]
    for K, tol in tols:
        _, _, info = ba.solve_step(lam, max_iters=200, rel_tol=tol)
        assert info["status"] == 0 and info["iterations"] == K and info["rel_residual"] <= tol, (kind, K, tol, info)
    ba.close()


# ---- 6. the converged step is the dense solution -------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("kind", KINDS)
def test_converged_step_is_the_dense_direct_solve(env, kind, lam):
    """test_gpu_schur_step.test_solve_accuracy's criteria, scaled by the condition number of the damped system"""
    ba = _load(_dome("bal"))
    ba.set_preconditioner(kind)
    ref = _lin(ba, np.float64)
    dc, dp, info = ba.solve_step(lam, max_iters=5000, rel_tol=1e-12)
    dc, dp = _np(dc), _np(dp)
    assert info["status"] == 0 and info["rel_residual"] <= 1e-12, info
    if ("kappa", lam) not in _cache:
        _cache[("kappa", lam)] = _kappa(ref, lam)
    kappa = _cache[("kappa", lam)]
    tol_res = max(1e-9, 1e3 * EPS * kappa)
    res, g = ref.damped_residual(lam, dc, dp)
    wc, wp = ref.direct(lam)
    d, w = np.concatenate([dc.ravel(), dp.ravel()]), np.concatenate([wc.ravel(), wp.ravel()])
    print("COUPLED dense %s lam=%g: kappa %.3g, %d iterations, |res| / |g| %.3g, |d - w| / |w| %.3g"
          % (kind, lam, kappa, info["iterations"], np.linalg.norm(res) / np.linalg.norm(g), np.linalg.norm(d - w) / np.linalg.norm(w)))
    assert np.linalg.norm(res) <= tol_res * np.linalg.norm(g), (kind, lam, kappa)
    assert np.linalg.norm(d - w) <= max(1e-8, kappa * tol_res) * np.linalg.norm(w), (kind, lam, kappa)
    md = float(_lin(ba).model_decrease(dc, dp))
    assert md > 0 and abs(info["model_decrease"] - md) <= 1e-10 * md, (info["model_decrease"], md)
    ba.close()


# ---- 7. under Cauchy ------------------------------------------------------------------------------------------------------------
def _cauchy(P):
    uv, pick = SC.dome_scaled_observations(P)
    ba = _load(P, uv)
    r = ba.residual_jacobian()[0]
    a = SC.cauchy_scale(r)
    w = B.weights("cauchy", a, r).astype(np.float64)
    assert w[pick].min() < 0.05 and np.median(w[~pick]) > 0.7, (w[pick].min(), np.median(w[~pick]))     # the weights differ widely
    return ba, a


def test_blocks_and_operator_under_cauchy(env):
    P = _dome("bal")
    ba, a = _cauchy(P)
    la = ("cauchy", a)
    nc, npt = ba.num_cameras(), ba.num_points()
    r, Jc, Jp = ba.residual_jacobian()
    wr, wJc, wJp = B.reweighted("cauchy", a, r, Jc, Jp)
    ref = NR.blocks(wr.astype(np.float64), wJc.astype(np.float64), wJp.astype(np.float64), SC.cam_of(ba.row_ptr),
                    ba.pt_idx.astype(np.int64), nc, npt)
    lam = 1e-2
    M = _device_blocks(env, ba, True, lam, loss=la)
    assert not _bits(M, _device_blocks(env, ba, True, lam))                  # the weights did something
    ba.set_loss(*la)
    U, gc, V, gp, s = ba.normal_equations()
    for dev_a, key, S, k in ((U, "U", "SU", "kc"), (gc, "gc", "Sgc", "kc"), (V, "V", "SV", "kp"), (gp, "gp", "Sgp", "kp")):
        x = NR.excess(_np(dev_a), ref[key], ref[S], ref[k] + _WEIGHT_OPS)    # test_gpu_robust_loss.py's count of the weighting's roundings
        print("COUPLED cauchy blocks %s: %.3g x the bound" % (key, x))
        assert x <= 1.0, (key, x)
    Q = _lin(ba, loss=la)
    SC.check_blocks(M, Q, lam, "dome cauchy", runs=8)
    _operator(env, ba, True, Q, "dome cauchy", loss=la)
    ba.close()


@pytest.mark.parametrize("kind", KINDS)
def test_pcg_iterates_under_cauchy(env, kind):
    ba, a = _cauchy(_dome("bal"))
    ba.set_loss("cauchy", a)
    ba.set_preconditioner(kind)
    lam, ks = 1e-2, SC.DOME_KS_SHORT
    Q, ref = _reference(("cauchy", kind), ba, lam, ks, kind, loss=("cauchy", a))
    SC.check_iterates(ba, Q, ref, lam, ks, tag="coupled cauchy " + kind, label="PCGREF")
    ba.close()


# ---- 8. under a mask ------------------------------------------------------------------------------------------------------------
def _masked_iterates(ba, cm, pm, lam, ks, kind, key, tag, loss=None):
    Q, ref = _reference(key, ba, lam, ks, kind, loss=loss, mask=(cm, pm))
    SC.check_iterates(ba, Q, ref, lam, ks, tag=tag, label="PCGREF")
    free = ~SC.unpack(cm)
    for k in ks:
        assert not ref["x"][k][~free].any() and not ref["dp"][k][pm].any()       # the reference's own are exact zeros
        dc, dp, _ = ba.solve_step(lam, max_iters=k, rel_tol=0.0)
        SC.assert_zeros(_np(dc), _np(dp), cm, pm, (tag, lam, k))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_pcg_iterates_under_a_mask(env, kind, mode):
    P = _dome(mode)
    ba = _load(P)
    cm, pm = SC.dome_mask(P)
    assert cm[0] == SC.POSE and (cm[1::2] & SC.INTRINSICS == SC.INTRINSICS).all() and (cm == SC.ALL).sum() == 1
    assert pm[DOME_CROWDED] and pm.sum() == 2
    ba.set_preconditioner(kind)
    ba.set_constant(cm, pm)
    _masked_iterates(ba, cm, pm, 1e-2, SC.DOME_KS_SHORT, kind, ("mask", kind, mode), "coupled mask %s %s" % (kind, mode))
    assert ba.preconditioner_fallbacks() == 0
    ba.close()


def test_cauchy_mask_and_schur_jacobi_together(env):
    P = _dome("bal")
    ba, a = _cauchy(P)
    cm, pm = SC.dome_mask(P)
    ba.set_loss("cauchy", a)
    ba.set_preconditioner("schur_jacobi")
    ba.set_constant(cm, pm)
    _masked_iterates(ba, cm, pm, 1e-2, SC.DOME_KS_SHORT, "schur_jacobi", ("cauchy mask",), "coupled cauchy mask schur_jacobi",
                     loss=("cauchy", a))
    ba.close()


@pytest.mark.parametrize("mode", MODES)
def test_apply_step_leaves_constant_bits_untouched(env, mode):
    P = _dome(mode)
    ba = _load(P)
    cm, pm = SC.dome_mask(P)
    ba.set_constant(cm, pm)
    m = SC.unpack(cm)
    b0, x0 = ba.cameras_bal(), ba.points()                       # state mode: the bits to_vec produces
    dc, dp, _ = ba.solve_step(1e-3)
    SC.assert_zeros(_np(dc), _np(dp), cm, pm, mode)
    ba.apply_step(dc, dp)
    b1, x1 = ba.cameras_bal(), ba.points()
    assert _bits(b1[m], b0[m]) and _bits(x1[pm], x0[pm])
    assert _bits(b1[~m], (b0 + _np(dc))[~m]) and _bits(x1[~pm], (x0 + _np(dp))[~pm])      # the free entries took the step
    kc = np.diff(ba.row_ptr.astype(np.int64))
    kp = np.bincount(ba.pt_idx.astype(np.int64), minlength=ba.num_points())
    moved_c = (b1 != b0).any(axis=1)
    assert moved_c[(kc > 0) & (cm != SC.ALL)].all() and not moved_c[kc == 0].any() and not moved_c[cm == SC.ALL].any()
    assert (x1 != x0).any(axis=1)[(kp > 0) & ~pm].all()
    ba.close()


# ---- 9. duplicates the project makes itself ----------------------------------------------------------------------------------
JOIN_PERCENT, JOIN_SEED = 0.3, 1


def test_joined_landmarks_give_a_camera_one_point_twice(env):
    from city2ba_amd import noise as N
    g, _ = _make("small grid culled")
    ba = N.join_landmarks(g, JOIN_PERCENT, seed=JOIN_SEED)       # a new problem, state mode
    g.close()
    Q = _lin(ba)
    assert PR.has_duplicate_pairs(Q)
    key = Q.cam * Q.n_pts + Q.pt
    print("COUPLED joined landmarks: %d cameras, %d points, %d observations, %d repeated pairs"
          % (Q.n_cam, Q.n_pts, len(key), len(key) - len(np.unique(key))))
    for lam in (1e-4, 1.0):
        SC.check_blocks(_device_blocks(env, ba, False, lam), Q, lam, "joined grid", runs=8)
    ba.set_preconditioner("schur_jacobi")
    lam, ks = 1e-2, (0, 1, 2, 3)
    Q, ref = _reference(("joined",), ba, lam, ks, "schur_jacobi")
    SC.check_iterates(ba, Q, ref, lam, ks, tag="coupled joined grid schur_jacobi", label="PCGREF")
    assert ba.preconditioner_fallbacks() == 0
    ba.close()


# ---- 10. determinism ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("kind", KINDS)
def test_two_solves_give_the_same_bits(env, kind, masked):
    P = _dome("state")
    out = []
    for _ in range(2):
        ba = _load(P)
        ba.set_preconditioner(kind)
        if masked:
            ba.set_constant(*SC.dome_mask(P))
        for _again in range(2):                                  # the same handle again, and a fresh one
            dc, dp, info = ba.solve_step(1e-4, max_iters=25, rel_tol=0.0)
            out.append((_np(dc).copy(), _np(dp).copy(), info))
        ba.close()
    assert out[0][2]["iterations"] == 25
    for o in out[1:]:
        assert _bits(o[0], out[0][0]) and _bits(o[1], out[0][1]) and o[2] == out[0][2]


# ---- 11. one LM run -------------------------------------------------------------------------------------------------------------
def test_levenberg_marquardt_reaches_the_hosts_error(env):
    """Ten iterations from the moved start, loaded in state mode.  The error falls on every accepted step and ends within
    a factor of the noise floor (the error of the state the observations were made from).  The factor comes from the
    host: _solvecheck.host_lm runs the same loop with the oracle's Jacobian and a dense direct solve of every damped
    system, and its final error over the noise floor, with 10 % of margin for the device's PCG stopping at a relative
    residual of 1e-8 instead of solving exactly, is the factor."""
    from city2ba_amd.solve import levenberg_marquardt
    P = _dome("state")
    host = SC.host_lm(P, 10)
    floor = _load(dict(P, bal9=P["true_bal9"], bal=True, pts=P["true_pts"]))
    e_floor = floor.total_reprojection_error(2.0) ** 2
    floor.close()
    factor = 1.1 * host[-1] / e_floor
    ba = _load(P)
    hist = levenberg_marquardt(ba, 10, lam=1e-4, max_iters=500, rel_tol=1e-8)
    errs = [h["error"] for h in hist] + [hist[-1]["error_after"]]
    print("COUPLED lm: device %s\nCOUPLED lm: host %s; noise floor %.6e, factor %.4f, accepted %s"
          % (["%.6e" % e for e in errs], ["%.6e" % e for e in host], e_floor, factor, [h["accepted"] for h in hist]))
    assert len(hist) == 10 and hist[0]["accepted"] and all(h["status"] in (0, 1) for h in hist)
    for k, h in enumerate(hist):
        assert errs[k + 1] < errs[k] if h["accepted"] else errs[k + 1] == errs[k], (k, errs)
    assert abs(errs[0] - host[0]) <= 1e-9 * host[0]
    assert errs[-1] <= factor * e_floor, (errs[-1], factor, e_floor)
    ba.close()
