"""The similarity alignment without a device: the reference of tests/_alignref.py against a brute restatement on clouds
moved by a known similarity, the library's host arithmetic (c2b_similarity_from_moments: Umeyama's closed form over a one-sided
Jacobi SVD) against the reference within the perturbation bound of the polar factor, and the trimming rules on the dome."""
import numpy as np
import pytest

import __graft_entry__ as entry
import _alignref as A
from _problems import noise_problem

U = A.U


@pytest.fixture(scope="module")
def L():
    entry.build()
    from city2ba_amd import _lib
    _lib.lib()
    return _lib


def _clouds():
    """(label, x, y, expected status, residual-free): x a cloud, y = the known similarity of it (or of its mirror image)"""
    P = noise_problem(40, 60, seed=21)
    general = np.concatenate([A.centers(P["cams15"]).astype(np.float64), P["pts"]])
    planar = noise_problem(0, 60, seed=22, variant="planar")["pts"]
    assert np.all(planar[:, 1] == planar[0, 1])
    line = np.outer(np.linspace(-3.0, 5.0, 20), [1.0, -2.0, 0.5]) + [4.0, 1.0, -2.0]
    out = [("general", general, A.move(general), A.OK, True),
           ("mirrored", general, A.move(general * [1.0, 1.0, -1.0]), A.OK, False),
           ("planar", planar, A.move(planar), A.OK, True),
           ("three", general[:3], A.move(general[:3]), A.OK, True),
           ("collinear", line, A.move(line), A.DEGENERATE, True),
           ("coincident", np.tile(general[:1], (5, 1)), A.move(np.tile(general[:1], (5, 1))), A.DEGENERATE, True),
           ("two", general[:2], A.move(general[:2]), A.TOO_FEW, True),
           ("none", general[:0], general[:0], A.TOO_FEW, True)]
    return out


CLOUDS = _clouds()


@pytest.mark.parametrize("case", CLOUDS, ids=[c[0] for c in CLOUDS])
def test_reference_recovers_the_known_similarity_and_agrees_with_a_brute_restatement(case):
    label, x, y, want, exact = case
    st, s, R, t, sig, eps = A.fit(x, y)
    assert st == want
    if st != A.OK:
        assert s == 1.0 and np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))       # the identity
        return
    assert abs(np.linalg.det(R) - 1.0) < 1e-14 and np.abs(R.T @ R - np.eye(3)).max() < 1e-15            # a proper rotation, always
    if exact:
        # y was rounded once from the exact image: the data are off by u |y| per coordinate, the fit by no more than a few times that
        scale_y = np.abs(y).max()
        assert abs(s - A.S0) < 64 * U * A.S0 * scale_y / np.sqrt(sig[1] / s), label
        assert np.abs(R - A.R0).max() < 64 * U * scale_y / np.sqrt(sig[1] / s)
        assert np.abs(t - A.T0).max() < 256 * U * scale_y * max(1.0, np.abs(x).max() / np.sqrt(sig[1] / s))
        assert A.errors(x, y, s, R, t).max() < 64 * U * scale_y
    else:
        assert eps == -1.0                                    # det(U V^T) < 0: the reflection is refused, a residual stays
        assert A.errors(x, y, s, R, t).max() > 1.0
    if len(x) >= 4 and label != "planar":                    # Horn's quaternion form: the same minimiser by another route
        sb, Rb, tb = A.fit_brute(x, y)
        assert abs(sb - s) < 1e-12 * s and np.abs(Rb - R).max() < 1e-12 and np.abs(tb - t).max() < 1e-10


@pytest.mark.parametrize("scale", (True, False))
@pytest.mark.parametrize("case", CLOUDS, ids=[c[0] for c in CLOUDS])
def test_similarity_from_moments_against_the_reference(L, case, scale):
    """the library's closed form on the SAME f64 moments the reference factors: R within 2 |dSigma|_F / (sig_2 + eps sig_3) with
    |dSigma|_F = 64 u |Sigma|_F for the factorisation's own rounding, s and t within that bound propagated to first order"""
    label, x, y, want, _ = case
    m = A.moments(x, y)
    n = m["n"]
    mx, my = m["mean_x"].astype(np.float64), m["mean_y"].astype(np.float64)
    vx, vy = (float(m["sxx"] / n), float(m["syy"] / n)) if n else (0.0, 0.0)
    cov = (m["sxy"] / n).astype(np.float64) if n else np.zeros((3, 3))
    st, s, R, t = L.similarity_from_moments(n, mx, my, vx, vy, cov, scale)
    rs, rsc, rR, rt, sig, eps = A.fit_from_moments(n, mx, my, vx, cov, scale)
    assert st == rs == want
    if st != A.OK:
        assert s == 1.0 and np.array_equal(R, np.eye(3)) and np.array_equal(t, np.zeros(3))
        return
    d_sigma = 64 * U * np.sqrt((cov * cov).sum())
    m64 = dict(m, mean_x=mx, mean_y=my)
    dR, ds, dt = A.fit_bounds(m64, sig, eps, rsc, d_sigma)
    print("%s: |dR|_F %.3g (bound %.3g)  ds %.3g (%.3g)  |dt| %.3g (%.3g)" % (label, np.sqrt(((R - rR) ** 2).sum()), dR, abs(s - rsc), ds,
                                                                            np.sqrt(((t - rt) ** 2).sum()), dt))
    assert np.sqrt(((R - rR) ** 2).sum()) <= dR
    assert np.linalg.det(R) > 0 and np.sqrt(((R.T @ R - np.eye(3)) ** 2).sum()) <= 16 * U
    if scale:
        assert abs(s - rsc) <= ds
    else:
        assert s == 1.0                                      # exactly
    assert np.sqrt(((t - rt) ** 2).sum()) <= dt


def test_similarity_from_moments_refuses_bad_arguments(L):
    import ctypes as C
    T, st = L.Similarity(), C.c_int(7)
    z3, z9 = np.zeros(3), np.zeros(9)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f = L.lib().c2b_similarity_from_moments
    assert f(5, None, p(z3), 1.0, 1.0, p(z9), 1, C.byref(T), C.byref(st)) == L.ERR_INVALID_ARGUMENT
    assert f(5, p(z3), p(z3), 1.0, 1.0, p(z9), 1, None, C.byref(st)) == L.ERR_INVALID_ARGUMENT
    assert f(-1, p(z3), p(z3), 1.0, 1.0, p(z9), 1, C.byref(T), C.byref(st)) == L.ERR_INVALID_ARGUMENT
    assert f(5, p(z3), p(z3), float("nan"), 1.0, p(z9), 1, C.byref(T), C.byref(st)) == L.ERR_INVALID_ARGUMENT
    assert st.value == 7                                     # nothing written


def test_finish_moments_moves_the_sums_from_the_pivot_to_the_mean(L):
    """c2b_align_finish_moments on sums formed in long double about a pivot that is NOT the mean (the device's pivot is the mean rounded
    to a double): the means and the eleven centred moments come out as the reference's, on the offset cloud too"""
    for variant in (None, "offset"):
        x = noise_problem(0, 50, seed=31, variant=variant)["pts"]
        y = A.move(x)
        m = A.moments(x, y)
        px, py = m["mean_x"].astype(np.float64) + 3e-7, m["mean_y"].astype(np.float64) - 2e-7       # a pivot off by far more than a rounding
        dx, dy = x.astype(A.LD) - px, y.astype(A.LD) - py
        mom = np.concatenate([[(dx * dx).sum(), (dy * dy).sum()], np.einsum("ni,nj->ij", dy, dx).ravel(), dx.sum(0), dy.sum(0), px, py]).astype(np.float64)
        means = np.concatenate([[50.0], x.sum(0), y.sum(0)])
        got = L.align_finish_moments(means, mom)
        assert got["n"] == 50
        assert np.all(np.abs(got["mean_x"] - m["mean_x"]) <= 4 * U * np.abs(m["mean_x"])) and np.all(np.abs(got["mean_y"] - m["mean_y"]) <= 4 * U * np.abs(m["mean_y"]))
        # the inputs were rounded once (u of each sum about the pivot); the correction itself is exact to a few u of the result
        tol = lambda ref, mag: 8 * U * (np.abs(ref) + mag)
        assert abs(got["var_x"] - m["sxx"] / 50) <= tol(m["sxx"] / 50, mom[0] / 50)
        assert abs(got["var_y"] - m["syy"] / 50) <= tol(m["syy"] / 50, mom[1] / 50)
        assert np.all(np.abs(got["cov"] - m["sxy"] / 50) <= tol(m["sxy"] / 50, np.abs(mom[2:11]).reshape(3, 3) / 50))


def test_trimming_flags_exactly_the_displaced_cameras_of_the_dome():
    """81 true centres + N(0, 1e-3), five displaced by 5 units, against the similarity of the truth: with max_dist = 0.5 the first fit is
    pulled away (35 of 81 within reach), the second set is exactly the 76, the third repeats it"""
    x, y = A.dome_trim_case(5.0)
    r = A.trim(x, y, 0.5, 3)
    assert r["status"] == A.OK and r["refits"] == 2
    assert [int(s.sum()) for s in r["sets"]] == [35, 76, 76]
    assert sorted(np.flatnonzero(~r["final"])) == sorted(A.DOME_DISPLACED)
    assert abs(r["s"] - A.S0) < 1e-4 * A.S0                    # (measured: 2.9e-5, the 1e-3 noise over a cloud of radius ~11)
    one = A.trim(x, y, 0.5, 1)                                 # one re-fit only: the transform of the 35
    assert one["refits"] == 1 and int(one["final"].sum()) == 35


def test_trimming_reports_an_emptied_set():
    """displaced by 50 units the five pull the least-squares start so far that nothing is within 0.5: TOO_FEW, the first fit's transform"""
    x, y = A.dome_trim_case(50.0)
    r = A.trim(x, y, 0.5, 3)
    st, s, R, t, _, _ = A.fit(x, y)
    assert r["status"] == A.TOO_FEW and r["refits"] == 0
    assert [int(k.sum()) for k in r["sets"]] == [0] and int(r["final"].sum()) == 0
    assert r["s"] == s and np.array_equal(r["R"], R) and np.array_equal(r["t"], t)


def test_rotation_error_keeps_small_angles_and_its_bound_covers_pi():
    """the chord form against the angles the cameras were turned by, and the first-order bound the device test uses"""
    P = noise_problem(6, 0, seed=23)["cams15"]
    rng = np.random.default_rng(5)
    angles = np.array([0.0, 1e-9, 1e-4, 1.0, np.pi - 1e-6, np.pi])
    turned = P.copy()
    for k, a in enumerate(angles):
        Rc = P[k, :9].reshape(3, 3).T.astype(A.LD)
        turned[k, :9] = (A.rotation(rng.normal(size=3), a).astype(A.LD) @ Rc).T.reshape(9).astype(np.float64)
    th, q = A.rotation_errors(turned, P, np.eye(3))
    b = A.rotation_error_bound(q)
    # the inputs are rounded to f64 (u per entry): the angle is the one applied within the same bound
    assert np.all(np.abs(th.astype(np.float64) - angles) <= b + 8 * U), (th - angles, b)
    assert abs(float(th[1]) - 1e-9) < 1e-6 * 1e-9
    assert b[1] < 4e-15 and b[3] < 1e-14 and b[5] < 1e-7       # a few u where the chord is well conditioned, ~sqrt(u) at pi
