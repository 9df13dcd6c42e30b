"""Checkers the solver's GPU tests share (test_gpu_schur_pcg, test_gpu_schur_jacobi, test_gpu_constant, test_gpu_coupled)
and the inputs test_coupled_problem.py and test_gpu_coupled.py must agree on: a device solve held to a reference PCG
iterate by iterate, the Schur-Jacobi blocks held to theirs camera by camera, the reference problem of a constant mask,
and for tests/_problems.py's dome_problem the compared iterates, the mask, the scaled observations and the host
Levenberg-Marquardt loop.  numpy and the references only: nothing here touches a device."""
import numpy as np

import _precondref as PR
import _robustref as B
import _schurref as R

EPS = R.EPS


def over(err, bound):
    return err / bound if bound > 0 else (0.0 if err == 0 else np.inf)


def rows_over(err, scale, tol):
    """per row: |err_row| / (tol |scale_row|), 0 where both are 0"""
    err = np.linalg.norm(np.asarray(err, dtype=np.float64).reshape(len(err), -1), axis=1)
    scale = tol * np.linalg.norm(np.asarray(scale, dtype=np.float64).reshape(len(scale), -1), axis=1)
    return np.array([over(e, s) for e, s in zip(err, scale)])


def sum_sq(P):
    r = P.r.astype(R.LD)
    return np.sum(r * r)


def model_tol(P, dc, dp):
    """64 eps x the absolute-value scale of the per-observation model terms -(2r + e).e and their sum"""
    dc, dp = np.abs(np.asarray(dc, dtype=np.float64)), np.abs(np.asarray(dp, dtype=np.float64))
    ae = np.einsum("nia,na->ni", np.abs(P.Jc), dc[P.cam]) + np.einsum("nia,na->ni", np.abs(P.Jp), dp[P.pt])
    ar = np.abs(P.r.astype(np.float64))
    return 64 * EPS * float(np.sum((2 * ar + 2 * ae) * ae))


def check_iterates(ba, P, ref, lam, ks, tag="", label="PCGREF"):
    """solve_step(lam, k, 0) against the reference PCG `ref` (of _schurref.pcg / _precondref.pcg on the longdouble Problem
    P, run to max(ks) at rel_tol 0) for every k in ks: x, dp, the recurrence residual and the energy within the bounds
    the reference returns, the energy falling where the reference's does by more than its bounds, sum_sq, and the model
    decrease.  The worst |err| / bound per quantity is printed.  Returns the reference."""
    assert ref["status"] == 1 and ref["iterations"] == max(ks), (ref["status"], ref["iterations"])
    b = ref["bound"]
    worst = dict(x=0.0, dp=0.0, rel=0.0, energy=0.0, model=0.0)
    e_prev = k_prev = None
    for k in ks:
        dc, dp, info = ba.solve_step(lam, max_iters=k, rel_tol=0.0)
        dc, dp = dc.cpu().numpy(), dp.cpu().numpy()
        assert info["status"] == 1 and info["iterations"] == k, (tag, k, info)
        ex = over(float(np.linalg.norm(dc - ref["x"][k].astype(np.float64))), b["x"][k])
        ed = over(float(np.linalg.norm(dp - ref["dp"][k].astype(np.float64))), b["dp"][k])
        er = over(abs(info["rel_residual"] - float(ref["rel"][k])), b["rel"][k])
        en = R.energy(P, lam, dc)
        ee = over(abs(float(en - ref["energy"][k])), b["energy"][k])
        for key, v in (("x", ex), ("dp", ed), ("rel", er), ("energy", ee)):
            worst[key] = max(worst[key], v)
            assert v <= 1.0, (tag, lam, k, key, v, info)
        if e_prev is not None and float(ref["energy"][k_prev] - ref["energy"][k]) > b["energy"][k] + b["energy"][k_prev]:
            assert en < e_prev, (tag, lam, k, float(en), float(e_prev))
        e_prev, k_prev = en, k
        ss = float(sum_sq(P))
        assert abs(info["sum_sq"] - ss) <= 1e-13 * ss, (tag, k, info["sum_sq"], ss)
        md = float(P.model_decrease(dc, dp))
        em = over(abs(info["model_decrease"] - md), model_tol(P, dc, dp))
        worst["model"] = max(worst["model"], em)
        assert em <= 1.0, (tag, lam, k, info["model_decrease"], md)
    print("%s %s lam=%g worst |err|/bound %s" % (label, tag, lam, {k: "%.3g" % v for k, v in worst.items()}))
    return ref


def crossing_tols(ref, n):
    """up to n thresholds, each between rel[K - 1] and rel[K] of a first crossing K >= 1 of the reference, and no rel[j],
    j <= K, within 1e-6 of it or within the reference's bound of it"""
    rel = np.array([float(v) for v in ref["rel"]])
    margin = np.asarray(ref["bound"]["rel"])
    out = []
    for K in range(1, len(rel)):
        if not rel[K] < rel[K - 1]:
            continue
        tol = np.sqrt(rel[K - 1] * rel[K])
        if (rel[:K] > tol).all() and rel[K] <= tol and (np.abs(rel[:K + 1] - tol) > np.maximum(1e-6 * tol, margin[:K + 1])).all():
            out.append((K, tol))
    return out[::max(1, len(out) // n)][:n]


def check_blocks(M, P, lam, tag, runs):
    """device Schur-Jacobi blocks M [n_cam, 9, 9] against _precondref.blocks_bound, camera by camera in the Frobenius
    norm; both triangles the same bits.  Returns |err| / bound per camera."""
    ref, bound, _ = PR.blocks_bound(P, lam, runs=runs)
    err = np.linalg.norm(M - ref.astype(np.float64), axis=(1, 2))
    ov = np.array([over(e, b) for e, b in zip(err, bound)])
    print("SJREF blocks %s lam=%g n_cam=%d worst |err|/bound %.3g" % (tag, lam, P.n_cam, float(ov.max())))
    assert np.isfinite(M).all() and float(ov.max()) <= 1.0, (tag, lam, float(ov.max()), int(ov.argmax()))
    Mt = np.ascontiguousarray(M.transpose(0, 2, 1))
    assert np.ascontiguousarray(M).tobytes() == Mt.tobytes(), (tag, "the two triangles differ")
    return ov


# ---- constant masks: the reference problem is that of J~, J with the constant columns set to zero -----------------------
def unpack(cm):
    return ((np.asarray(cm, dtype=np.uint16)[:, None] >> np.arange(9, dtype=np.uint16)) & 1).astype(bool)


def masked_jacobian(Jc, Jp, cam, pt, cm, pm):
    """(Jc~, Jp~): the columns of constant camera parameters (uint16 [n_cam]) and constant points (bool [n_pts]) zeroed"""
    Jc = np.where(unpack(cm)[cam][:, None, :], 0.0, np.asarray(Jc).reshape(len(cam), 2, 9))
    Jp = np.where(np.asarray(pm, dtype=bool)[pt][:, None, None], 0.0, np.asarray(Jp).reshape(len(pt), 2, 3))
    return Jc, Jp


def assert_zeros(dc, dp, cm, pm, tag):
    dc, dp = np.asarray(dc), np.asarray(dp)
    assert (dc[unpack(cm)] == 0.0).all(), (tag, "a constant camera parameter moved")
    assert (dp[np.asarray(pm, dtype=bool)] == 0.0).all(), (tag, "a constant point moved")


# ---- dome_problem: what its CPU test asserts and its GPU tests use ------------------------------------------------------
# The iterates compared per (preconditioner, lam).  At each of them the reference's own rerun-derived bound on x and dp is
# at most DOME_CAP of the iterate's norm (test_coupled_problem.py asserts it with the oracle's Jacobian, the GPU tests
# with the device's): at lam = 1e-4 both preconditioners stay below 3e-7 through 40 iterations, at lam = 1 the bound is
# its floor, 1e-13, throughout; lam = 1 stops at 12, where the residual has fallen to 1e-12 of |b| and further iterates
# no longer differ from one another by more than rounding.
DOME_CAP = 1e-6
DOME_KS = {("block_jacobi", 1e-4): (0, 1, 2, 3, 5, 8, 13, 21, 34), ("schur_jacobi", 1e-4): (0, 1, 2, 3, 5, 8, 13, 21, 34),
           ("block_jacobi", 1.0): (0, 1, 2, 3, 5, 8, 12), ("schur_jacobi", 1.0): (0, 1, 2, 3, 5, 8, 12)}
DOME_KS_SHORT = (0, 1, 2, 3, 5, 8)                  # the variants (loss, mask, joined landmarks): lam = 1e-2


def cap_excess(ref, ks):
    """the largest bound / (DOME_CAP x the iterate's norm) over x and dp at the iterates ks (an iterate of norm 0 must
    have a bound of 0)"""
    worst = 0.0
    for key in ("x", "dp"):
        for k in ks:
            worst = max(worst, over(ref["bound"][key][k], DOME_CAP * float(np.linalg.norm(ref[key][k].astype(np.float64)))))
    return worst


ROTATION, TRANSLATION, POSE, FOCAL, K1, K2, INTRINSICS, ALL = 0x007, 0x038, 0x03f, 0x040, 0x080, 0x100, 0x1c0, 0x1ff


def dome_mask(P):
    """(uint16 [n_cam], bool [n_pts]): the gauge on camera 0 (its pose), the intrinsics of every other camera, one camera
    with a 257-long row wholly constant, nothing on the rest; the crowded point and one point seen once constant"""
    from _problems import DOME_CROWDED
    lengths = np.asarray(P["lengths"])
    cm = np.zeros(len(lengths), dtype=np.uint16)
    cm[1::2] = INTRINSICS
    cm[0] = POSE
    cm[int(np.flatnonzero(lengths == 257)[0])] = ALL
    kp = np.bincount(P["pt_idx"].astype(np.int64), minlength=len(P["pts"]))
    pm = np.zeros(len(P["pts"]), dtype=bool)
    pm[DOME_CROWDED] = True
    pm[int(np.flatnonzero(kp == 1)[0])] = True
    assert (cm == 0).any() and kp[DOME_CROWDED] > 64
    return cm, pm


def dome_scaled_observations(P, seed=5, frac=0.1, factor=30.0):
    """uv with the residual of a seeded `frac` of the observations scaled by `factor` (uv moved along its own residual
    from the noise-free projection), so that a robust loss's weights differ widely"""
    import oracle as O
    rng = np.random.default_rng(seed)
    proj = O.project_observations(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"])
    pick = rng.random(len(proj)) < frac
    uv = P["uv"].copy()
    uv[pick] = proj[pick] + factor * (uv[pick] - proj[pick])
    return uv, pick


def cauchy_scale(r):
    """twice the median residual norm, as test_gpu_robust_loss.py sets it"""
    return 2.0 * float(np.median(np.linalg.norm(np.asarray(r).reshape(-1, 2), axis=1)))


def cam_of(row_ptr):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))


def oracle_problem(P, dtype=np.float64, uv=None, loss=None, mask=None):
    """the _schurref.Problem of a dome_problem from the oracle's Jacobian of its mode, optionally with other
    observations, under loss = (name, scale) and under mask = (cm, pm)"""
    import oracle as O
    uv = P["uv"] if uv is None else uv
    if P["bal"]:
        r, Jc, Jp = O.residual_jacobian_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], uv)
    else:
        r, Jc, Jp = O.residual_jacobian(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], uv)
    return linearisation(r, Jc, Jp, P["row_ptr"], P["pt_idx"], len(P["bal9"]), len(P["pts"]), dtype, loss, mask)


def linearisation(r, Jc, Jp, row_ptr, pt_idx, n_cam, n_pts, dtype=np.float64, loss=None, mask=None):
    cam, pt = cam_of(row_ptr), np.asarray(pt_idx).astype(np.int64)
    if mask is not None:
        Jc, Jp = masked_jacobian(Jc, Jp, cam, pt, *mask)
    if loss is not None:
        return B.problem(loss[0], loss[1], r, Jc, Jp, cam, pt, n_cam, n_pts, dtype=dtype)
    return R.Problem(r, Jc, Jp, cam, pt, n_cam, n_pts, dtype=dtype)


def host_lm(P, iterations, lam=1e-4):
    """city2ba_amd.solve.levenberg_marquardt's loop on the host in bal mode: the oracle's Jacobian, the step by a dense
    direct solve of the damped system (Problem.direct), the same acceptance and the same update of the damping.  Returns
    the sums of squared residuals [iterations + 1]."""
    import oracle as O
    bal9, pts = P["bal9"].copy(), P["pts"].copy()
    n_cam, n_pts = len(bal9), len(pts)

    def lin(b9, X):
        r, Jc, Jp = O.residual_jacobian_bal(b9, X, P["row_ptr"], P["pt_idx"], P["uv"])
        return R.Problem(r, Jc, Jp, cam_of(P["row_ptr"]), P["pt_idx"].astype(np.int64), n_cam, n_pts)

    Q = lin(bal9, pts)
    e0, nu, out = float(np.sum(Q.r * Q.r)), 2.0, []
    out.append(e0)
    for _ in range(iterations):
        dc, dp = Q.direct(lam)
        Q1 = lin(bal9 + dc, pts + dp)
        e1 = float(np.sum(Q1.r * Q1.r))
        md = float(Q.model_decrease(dc, dp))
        rho = (e0 - e1) / md if md > 0.0 else -1.0
        if rho > 0.0 and e1 < e0:
            lam = min(max(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e-20), 1e32)
            nu = 2.0
            bal9, pts, Q, e0 = bal9 + dc, pts + dp, Q1, e1
        else:
            lam = min(max(lam * nu, 1e-20), 1e32)
            nu *= 2.0
        out.append(e0)
    return out
