"""The checker of tests/test_gpu_jacobian_entries.py, checked (CPU only):
  * tests/_jacref.py's longdouble reference against mpmath at 40 digits, entry by entry, on every family in both modes;
  * ... and against the 270 mpmath-differentiated golden pairs, to within the golden values' own rounding to f64;
  * the kernel's arithmetic (jacobian_obs + left_jacobian + from_rodrigues) restated in f64 in the kernel's order stays
    inside C E on about a million observations -- the bound is sound;
  * one-line mutations of that arithmetic land outside it -- the bound is tight enough to see them."""
import numpy as np
import pytest

import mpmath as mp

import _jacref as J
import oracle as O

FAM_MODES = [(f, m) for f in J.FAMILIES for m in ("bal", "state")]


def _cases(fam, mode, m, seed):
    """cameras [m, 9 or 15], X, w (state mode: the to_vec the J_l columns refer to), per observation"""
    bal9, cam_of, X, lab = J.family(fam, m, seed, mode)
    b = bal9[cam_of]
    if mode == "bal":
        return b, X, None, lab
    return O.camera_from_bal(b), X, b[:, 0:3].copy(), lab


# ---- mpmath ------------------------------------------------------------------------------------------------------
def _ld2mp(x):
    n, d = J.LD(x).as_integer_ratio()
    return mp.mpf(n) / d                       # d is a power of two: exact


def _mp_skew(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _mp_coeffs(w):
    th2 = w[0] ** 2 + w[1] ** 2 + w[2] ** 2
    if th2 == 0:
        return mp.mpf(1), mp.mpf(1) / 2, mp.mpf(1) / 6
    th = mp.sqrt(th2)
    return mp.sin(th) / th, (1 - mp.cos(th)) / th2, (th - mp.sin(th)) / (th2 * th)


def _mp_jac(R, t, intr, w, X):
    """Jc 2x9, Jp 2x3 at 40 digits: rotation columns -[R X]x J_l(w), R given (mp matrix)"""
    A, B, Cb = _mp_coeffs(w)
    K = _mp_skew(w)
    Jl = mp.eye(3) + B * K + Cb * K * K
    y = R * mp.matrix(X)
    q = y + mp.matrix(t)
    f, k1, k2 = intr
    px, py = -q[0] / q[2], -q[1] / q[2]
    n = px * px + py * py
    rad = 1 + k1 * n + k2 * n * n
    c = 2 * k1 + 4 * k2 * n
    M = mp.matrix([[rad + c * px * px, c * px * py], [c * px * py, rad + c * py * py]])
    P = mp.matrix([[-1 / q[2], 0, q[0] / q[2] ** 2], [0, -1 / q[2], q[1] / q[2] ** 2]])
    Aq = f * M * P
    Jw = Aq * (-_mp_skew(y)) * Jl
    Jp = Aq * R
    Jc = [[Jw[i, j] for j in range(3)] + [Aq[i, j] for j in range(3)] +
          [rad * [px, py][i], f * n * [px, py][i], f * n * n * [px, py][i]] for i in range(2)]
    return Jc, [[Jp[i, j] for j in range(3)] for i in range(2)]


def _mp_case(mode, cam, X, w):
    m = [mp.mpf(float(x)) for x in cam]
    if mode == "bal":
        wv = m[0:3]
        A, B, _ = _mp_coeffs(wv)
        K = _mp_skew(wv)
        R = mp.eye(3) + A * K + B * K * K
        return _mp_jac(R, m[3:6], m[6:9], wv, [mp.mpf(float(x)) for x in X])
    R = mp.matrix([[m[3 * c + r] for c in range(3)] for r in range(3)])
    return _mp_jac(R, m[9:12], m[12:15], [mp.mpf(float(x)) for x in w], [mp.mpf(float(x)) for x in X])


@pytest.mark.parametrize("fam,mode", FAM_MODES)
def test_reference_agrees_with_mpmath(fam, mode):
    """componentwise within 2^-60 of each entry's magnitude -- the larger of |entry| and E / u, the sum of the magnitudes it
    is computed from (an entry that cancels is only as well defined as its f64 inputs let it be: a near-plane point's
    q.z = (R X + t).z loses |X| / |q.z| of any finite precision).  The reference's error then stays below 2^-7 u of that
    sum: well inside the kernel's own tolerance C E.  Bal mode takes a different form -- the directional derivative of
    Rodrigues' formula against -[RX]x J_l(w) in mpmath --, so the identity between the two is checked too."""
    cams, X, w, _ = _cases(fam, mode, 200, seed=11)
    ref = J.reference_bal(cams, X) if mode == "bal" else J.reference_state(cams, w, X)
    _, Ec, _, Ep = J.bounds(mode, cams, X, w)
    worst, where = 0.0, None
    with mp.workdps(40):
        for i in range(len(X)):
            Jc, Jp = _mp_case(mode, cams[i], X[i], None if w is None else w[i])
            for got, want, E, key in ((ref["Jc"][i], Jc, Ec[i], "Jc"), (ref["Jp"][i], Jp, Ep[i], "Jp")):
                for a in range(2):
                    for b in range(len(want[a])):
                        d = abs(_ld2mp(got[a, b]) - want[a][b])
                        mag = max(abs(want[a][b]), mp.mpf(float(E[a, b])) / mp.mpf(J.U))
                        if d > 0 and (mag == 0 or d / mag > worst):
                            worst, where = (float(d / mag) if mag > 0 else float("inf")), (i, key, a, b)
    assert worst <= 2.0 ** -60, "%s/%s: worst difference from mpmath 2^%.1f of the entry's magnitude at %s" % (
        fam, mode, np.log2(worst), where)


def test_reference_agrees_with_golden_pairs(golden):
    """the 270 golden pairs (mpmath derivatives of the model, rounded to f64): within half an ulp of each golden value plus
    the reference's own 2^-60 of the entry's magnitude (as above)"""
    pairs = golden["pairs"]
    bal9 = np.array([p["bal9"] for p in pairs])
    X = np.array([p["X"] for p in pairs])
    ref = J.reference_bal(bal9, X)
    _, Ec, _, Ep = J.bounds("bal", bal9, X)
    for key, got, E in (("Jc", ref["Jc"], Ec), ("Jp", ref["Jp"], Ep)):
        got, E = got.reshape(len(pairs), -1), E.reshape(len(pairs), -1)
        want = np.array([p[key] for p in pairs])
        half_ulp = np.spacing(np.abs(want)) / 2
        err = np.abs(got - want.astype(J.LD)).astype(np.float64)
        tol = half_ulp + 2.0 ** -60 * np.maximum(np.abs(want), E / J.U)
        bad = np.argwhere(err > tol)
        assert len(bad) == 0, "%s: %d entries beyond half an ulp of the golden value, first %s (err %.3g, half ulp %.3g)" % (
            key, len(bad), bad[0], err[tuple(bad[0])], half_ulp[tuple(bad[0])])
        assert np.max(err[want != 0] / half_ulp[want != 0]) > 0.25        # the comparison is not vacuous


@pytest.mark.parametrize("fam,mode", FAM_MODES)
def test_restated_kernel_stays_inside_the_bound(fam, mode):
    """about a million observations in all (six family / mode pairs); the kernel's order, restated, inside C E everywhere"""
    cams, X, w, _ = _cases(fam, mode, 170_000, seed=29)
    ref = J.reference_bal(cams, X) if mode == "bal" else J.reference_state(cams, w, X)
    Jc, Ec, Jp, Ep = J.bounds(mode, cams, X, w)
    msg = (J.worst_report(Jc, ref["Jc"], Ec, J.COLS, "%s/%s Jc" % (fam, mode)) +
           J.worst_report(Jp, ref["Jp"], Ep, J.PCOLS, "%s/%s Jp" % (fam, mode)))
    assert not msg, msg
    # the bound is not vacuous: the worst entry uses a visible part of it
    assert max(J.ratio(Jc, ref["Jc"], Ec), J.ratio(Jp, ref["Jp"], Ep)) > 0.05


def test_exact_zeros_on_the_optical_axis():
    """p = 0 exactly (R = I, X = (-t0, -t1, .)): the f, k1, k2 and t2 columns are exactly 0 in the reference and the
    restatement"""
    bal9, cam_of, X, lab = J.family("geometry", 600, 3)
    ax = lab == "axis"
    assert ax.sum() > 50
    ref = J.reference_bal(bal9[cam_of][ax], X[ax])
    Jc = J.bounds("bal", bal9[cam_of][ax], X[ax])[0]
    for a in (ref["Jc"], Jc):
        assert np.all(a[:, :, 5:9] == 0)


# one-line changes of camera_math.hpp / kernels.hpp, restated: each must fall outside the bound of the kernel as it is
MUTATIONS = {
    "series_1e-1": "left_jacobian: series below t2 = 1e-1 instead of 1e-2",
    "a_series_short": "left_jacobian: the series of a cut after its t2^2 term",
    "rodrigues_threshold": "from_rodrigues: small-angle branch below theta2 = 1e-8 instead of f64::EPSILON",
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_mutations_fall_outside_the_bound(mutation):
    outside = 0
    for fam, mode in FAM_MODES:
        cams, X, w, _ = _cases(fam, mode, 20_000, seed=31)
        ref = J.reference_bal(cams, X) if mode == "bal" else J.reference_state(cams, w, X)
        Jc, Ec, Jp, Ep = J.bounds(mode, cams, X, w, (mutation,))
        outside += int(np.sum(J.excess(Jc, ref["Jc"], Ec) > 1.0)) + int(np.sum(J.excess(Jp, ref["Jp"], Ep) > 1.0))
    assert outside > 0, "%s (%s) stays inside C E everywhere" % (mutation, MUTATIONS[mutation])
