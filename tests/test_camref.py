"""The checker of tests/test_gpu_camera_reference.py, checked (CPU only):
  * tests/_camref.py's longdouble reference (log_ld, _jacref.exp_so3) against mpmath at 40 digits on a sample of every family:
    by log_ld's own definition, and -- independent of it -- mpmath's exp of log_ld's result against the matrix that went in;
  * the restated from_rodrigues / to_rodrigues / cm_center against the oracle: within E, bit-equal where no transcendental
    is involved;
  * the restatement stays inside E (no margin C) on every family -- the bound is honest -- and uses a visible part of it
    at every |w| of the `angles` family -- it is not slack where it matters;
  * one-line mutations of the restated arithmetic land outside C E -- the bound is tight enough to see them."""
import numpy as np
import pytest

import mpmath as mp

import _camref as R
import _jacref as J
import oracle as O

LD = J.LD
TWO60 = 2.0 ** -60


@pytest.fixture(scope="module")
def fams():
    return R.families()


def _ld2mp(x):
    n, d = LD(x).as_integer_ratio()
    return mp.mpf(n) / d


def _mp_exp(w):
    w = [x if isinstance(x, mp.mpf) else mp.mpf(float(x)) for x in w]
    th2 = w[0] ** 2 + w[1] ** 2 + w[2] ** 2
    K = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th2 == 0:
        return mp.eye(3) + K
    th = mp.sqrt(th2)
    return mp.eye(3) + mp.sin(th) / th * K + (1 - mp.cos(th)) / th2 * K * K


def _mp_log(Rcm):
    """the principal rotation vector (|w| <= pi) by log_ld's definition -- the quaternion of the largest candidate, the
    axis v / |v| -- with the angle through other functions: 2 asin(|v| / |q|) below pi / 2, 2 acos(q0 / |q|) above"""
    M = mp.matrix([[mp.mpf(float(Rcm[3 * c + r])) for c in range(3)] for r in range(3)])
    d = [M[0, 0], M[1, 1], M[2, 2]]
    cand = [1 + d[0] + d[1] + d[2], 1 + d[0] - d[1] - d[2], 1 - d[0] + d[1] - d[2], 1 - d[0] - d[1] + d[2]]
    k = max(range(4), key=lambda i: cand[i])
    a = [M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]
    s = {(1, 2): M[0, 1] + M[1, 0], (1, 3): M[0, 2] + M[2, 0], (2, 3): M[1, 2] + M[2, 1]}
    big = 2 * mp.sqrt(cand[k])
    q = [None] * 4
    q[k] = big / 4
    for j in range(4):
        if j != k:
            q[j] = (a[max(j, k) - 1] if min(j, k) == 0 else s[(min(j, k), max(j, k))]) / big
    if q[0] < 0:
        q = [-x for x in q]
    nv = mp.sqrt(q[1] ** 2 + q[2] ** 2 + q[3] ** 2)
    if nv == 0:
        return [mp.mpf(0)] * 3
    nq = mp.sqrt(q[0] ** 2 + nv ** 2)
    th = 2 * (mp.asin(nv / nq) if nv < q[0] else mp.acos(q[0] / nq))
    return [th * x / nv for x in q[1:]]


def _principal(w, other):
    """of the two representatives, the one with |w| <= pi"""
    n0, n1 = (w * w).sum(axis=1), (other * other).sum(axis=1)
    return np.where((n0 <= n1)[:, None], w, other)


def test_reference_agrees_with_mpmath(fams):
    """exp_so3 entry by entry within 2^-60 max(1, |w|), log_ld within 2^-60 |w|, on every |w| of `angles` and
    a sample of every other rotation family; log_ld(exp_so3(w)) returns w below pi"""
    worst_exp = worst_log = worst_rt = 0.0
    with mp.workdps(40):
        f = fams["angles"]
        pick = np.arange(0, len(f["bal9"]), 3)
        E = J.exp_so3(f["bal9"][pick, 0:3])
        for i, k in enumerate(pick):
            want = _mp_exp(f["bal9"][k, 0:3])
            # a rotation's entries are of size 1 and move by |dw|: the angle, rounded once, is known to |w| 2^-64
            scale = max(1.0, float(np.linalg.norm(f["bal9"][k, 0:3])))
            for r in range(3):
                for c in range(3):
                    worst_exp = max(worst_exp, float(abs(_ld2mp(E[i, r, c]) - want[r, c])) / scale)
        assert worst_exp <= TWO60, "exp_so3: 2^%.1f of max(1, |w|) from mpmath" % np.log2(worst_exp)
        for name in R.ROTATION_FAMILIES:
            cam = fams[name]["cam15"]
            pick = np.arange(0, len(cam), max(1, len(cam) // 120))
            w, other, _ = R.log_ld(cam[pick, 0:9])
            got = _principal(w, other)
            for i, k in enumerate(pick):
                want = _mp_log(cam[k, 0:9])
                scale = max(abs(x) for x in want)
                for c in range(3):
                    d = abs(_ld2mp(got[i, c]) - want[c])
                    if d > 0:
                        assert scale > 0, (name, k)
                        worst_log = max(worst_log, float(d / scale))
            assert worst_log <= TWO60, "%s log_ld: 2^%.1f of |w| from mpmath" % (name, np.log2(worst_log))
    # the round trip in longdouble alone: exp_so3 of the 9-vectors' w, log_ld of that matrix
    b = fams["angles"]["bal9"]
    nrm = np.sqrt((b[:, 0:3].astype(LD) ** 2).sum(axis=1))
    sel = (nrm > 0) & (nrm < np.pi - 1e-6)
    w, other, _ = R.log_ld(R.colmajor(J.exp_so3(b[sel, 0:3])))
    rel = (np.abs(_principal(w, other) - b[sel, 0:3].astype(LD)).max(axis=1) / nrm[sel]).astype(np.float64)
    worst_rt = float(rel.max())
    assert worst_rt <= TWO60, "log_ld(exp_so3(w)): 2^%.1f of |w| from w" % np.log2(worst_rt)
    print("[camref] reference against mpmath: exp 2^%.1f, log 2^%.1f of |w|; log(exp(w)) 2^%.1f of |w|"
          % tuple(np.log2(max(x, 1e-300)) for x in (worst_exp, worst_log, worst_rt)))


def _mp_exp_distance(w_ld, want):
    """max |exp(w) - want| over the entries, w a longdouble 3-vector taken exactly, want an mp matrix"""
    got = _mp_exp([_ld2mp(x) for x in w_ld])
    return max(abs(got[r, c] - want[r, c]) for r in range(3) for c in range(3))


def test_log_ld_inverts_mpmaths_exponential(fams):
    """independent of log_ld's algorithm: mpmath's exp of what log_ld returns -- of BOTH representatives -- is the matrix
    that went in.  A matrix within d of a rotation is reproduced to 16 d (log_ld moves by at most 8 d under such a change,
    _camref.to_vec; a rotation by sqrt 2 times that, plus d) + 2^-60 max(1, |w|):
      * the f64 matrices of every rotation family, d = max |R^T R - I| (0 on the cube: the sharp case);
      * rotations mpmath itself builds from the vectors of `angles` (every |w|, beyond pi included) and from vectors within
        0.3 of pi about x-, y- and z-dominated axes, rounded to longdouble: d = that rounding, ~2^-64."""
    worst = {}
    with mp.workdps(40):
        for name in R.ROTATION_FAMILIES:
            cam = fams[name]["cam15"]
            pick = np.arange(0, len(cam), max(1, len(cam) // 100))
            dl = R.defect(cam[pick, 0:9])
            w, other, _ = R.log_ld(cam[pick, 0:9])
            for i, k in enumerate(pick):
                M = mp.matrix([[mp.mpf(float(cam[k, 3 * c + r])) for c in range(3)] for r in range(3)])
                for rep in (w[i], other[i]):
                    tol = 16 * mp.mpf(float(dl[i])) + mp.mpf(TWO60) * max(1, float(np.abs(rep).max()))
                    d = _mp_exp_distance(rep, M)
                    assert d <= tol, "%s camera %d: exp(log_ld(R)) is %.3g from R (tolerance %.3g)" % (name, k, float(d), float(tol))
                    worst[name] = max(worst.get(name, 0.0), float(d / tol))
        rng = np.random.default_rng(41)
        ax = 0.45 * rng.normal(size=(60, 3))
        ax[np.arange(60), np.arange(60) % 3] = np.where(rng.random(60) < 0.5, -1.0, 1.0)
        near_pi = ax / np.linalg.norm(ax, axis=1, keepdims=True) * (np.pi + rng.uniform(-0.3, 0.3, 60))[:, None]
        ws = np.concatenate([fams["angles"]["bal9"][::2, 0:3], near_pi])
        for k, wv in enumerate(ws):
            M = _mp_exp(wv)
            Mld = np.array([[LD(mp.nstr(M[r, c], 30)) for c in range(3)] for r in range(3)])
            e = max(abs(_ld2mp(Mld[r, c]) - M[r, c]) for r in range(3) for c in range(3))
            w, other, _ = R.log_ld(R.colmajor(Mld[None, :, :]))
            for rep in (w[0], other[0]):
                tol = 16 * e + mp.mpf(TWO60) * max(1, float(np.abs(rep).max()))
                d = _mp_exp_distance(rep, M)
                assert d <= tol, "vector %d (|w| = %.17g): exp(log_ld(exp(w))) is %.3g from exp(w) (tolerance %.3g)" % (
                    k, float(np.linalg.norm(wv)), float(d), float(tol))
                worst["mpmath's"] = max(worst.get("mpmath's", 0.0), float(d / tol))
    print("[camref] exp(log_ld(R)) against R in mpmath, worst distance / tolerance: %s" % {k: "%.3g" % v for k, v in worst.items()})


def test_restatement_agrees_with_the_oracle(fams):
    """the oracle runs the same operations with libm's sin / cos / acos: bit-equal where none of them enters (the small-angle
    branch of from_rodrigues, the zero branch of to_rodrigues, t, the intrinsics, every centre), within E elsewhere"""
    for name, f in fams.items():
        cam = f["cam15"]
        W, E, masks = R.to_vec(cam, rotation=f["rotation"])
        got = O.camera_to_bal(cam)
        zero = masks[3]
        assert np.array_equal(got[zero, 0:3].view(np.uint64), W[zero].view(np.uint64)), name
        assert np.all(W[zero] == 0.0)
        assert np.array_equal(got[:, 3:9].view(np.uint64), cam[:, 9:15].view(np.uint64)), name
        assert np.all(np.abs(got[:, 0:3] - W) <= E + J.FLOOR), name
        c, _ = R.center(cam)
        assert np.array_equal(O.centers(cam).view(np.uint64), c.view(np.uint64)), name
    b = fams["angles"]["bal9"]
    Rv, Er, small = R.from_vec(b)
    got = O.camera_from_bal(b)
    assert small.sum() > 50 and (~small).sum() > 50
    assert np.array_equal(got[small, 0:9].view(np.uint64), Rv[small].view(np.uint64))
    assert np.array_equal(got[:, 9:15].view(np.uint64), b[:, 3:9].view(np.uint64))
    assert np.all(np.abs(got[:, 0:9] - Rv) <= Er + J.FLOOR)


def _to_vec_reference(f, dev, masks):
    """what a to_vec result `dev` of family f is judged against: log_ld's representative on the rotation families, the
    formula itself in longdouble (on the branches `masks` of the unmutated f64 run) on `scaled`"""
    cam = f["cam15"]
    if not f["rotation"]:
        return R.formula_ld(cam, masks)
    w, other, either = R.log_ld(cam[:, 0:9], R.defect(cam[:, 0:9]))
    return R.nearest(dev, w, other, either)


# |w| of `angles` whose to_vec is (next to) exactly zero: the restatement returns 0, the error is |w| or its distance from
# 2 pi (2.4e-16), and the bound is the cut-off's own 2 sqrt(eps) -- their ratio is that number over 3e-8 by definition
NEXT_TO_ZERO = ("0", "1e-300", "1e-160", "2pi")


def test_the_bound_is_honest_and_not_slack(fams):
    """|restated - reference| <= E, no C, on every family: to_vec, from_vec (`angles`), the centre's residual; and on `angles`
    the median |restated - reference| / E of every |w| label is at least 1e-3"""
    for name, f in fams.items():
        cam = f["cam15"]
        W, E, masks = R.to_vec(cam, rotation=f["rotation"])
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(E)), name
        ref = _to_vec_reference(f, W, masks)
        err = np.abs(W - ref).astype(np.float64)
        assert np.all(err <= E + np.abs(ref).astype(np.float64) * TWO60 + J.FLOOR), "%s: to_vec %.3g of E" % (name, R.ratio(W, ref, E))
        c, Ec = R.center(cam)
        res, scale = R.center_residual(cam, c)
        assert np.all(np.abs(res).astype(np.float64) <= R.center_bound(cam, Ec) + scale.astype(np.float64) * TWO60 + J.FLOOR), name
        print("[camref] %-8s to_vec worst |err|/E = %.3g, defect %.2e, quaternion branches %s, zeros %d" % (
            name, R.ratio(W, ref, E), R.defect(cam[:, 0:9]).max(), [int(m.sum()) for m in R.branch_masks(cam[:, 0:9])], int(masks[3].sum())))
        if name == "angles":
            for lab in R.ANGLE_NAMES:
                s = f["label"] == lab
                with np.errstate(divide="ignore", invalid="ignore"):
                    r = np.where(err[s] == 0, 0.0, err[s] / E[s]).max(axis=1)
                print("[camref]   |w| = %-10s median |err|/E = %.3g, worst |err| = %.3g" % (lab, np.median(r), err[s].max()))
                if lab in NEXT_TO_ZERO:
                    assert np.all(W[s] == 0.0) and err[s].max() <= 1e-15
                else:
                    assert np.median(r) >= 1e-3, lab
    b = fams["angles"]["bal9"]
    Rv, Er, _ = R.from_vec(b)
    ref = R.colmajor(J.exp_so3(b[:, 0:3]))
    assert np.all(np.abs(Rv - ref).astype(np.float64) <= Er + J.FLOOR), "from_vec %.3g of E" % R.ratio(Rv, ref, Er)
    print("[camref] angles   from_vec worst |err|/E = %.3g" % R.ratio(Rv, ref, Er))


def test_every_quaternion_branch_is_populated(fams):
    counts = [int(m.sum()) for m in R.branch_masks(fams["branches"]["cam15"][:, 0:9])]
    print("[camref] branches: trace / x / y / z = %s" % counts)
    assert min(counts) >= 100, counts
    # ... and the cube brings trace = 0 exactly, the ties and the zero branch
    cam = fams["cube"]["cam15"]
    tr = (cam[:, 0] + cam[:, 4]) + cam[:, 8]
    assert np.sum(tr == 0.0) >= 8 and np.sum((tr == -1.0) & (cam[:, 0] == cam[:, 4])) >= 1 and np.sum((tr == -1.0) & (cam[:, 4] == cam[:, 8])) >= 1
    assert np.all(R.to_vec(cam[fams["cube"]["label"] == "cube/0"])[2][3])


# one-line changes of camera_math.hpp, restated: each must fall outside C E of the arithmetic as it is
MUTATIONS = {
    "to_cutoff": ("to_rodrigues: cut-off 1 - q0^2 < 1e-8 instead of f64::EPSILON", None),
    "rodrigues_threshold": ("from_rodrigues: small-angle branch below theta2 = 1e-8 instead of f64::EPSILON", None),
    "sign_b1": ("cm_quat_from_mat: y = (m10 - m01) s on the m00 branch", None),
    "sign_b2": ("cm_quat_from_mat: z = (m21 - m12) s on the m11 branch", None),
    "sign_b3": ("cm_quat_from_mat: x = (m02 - m20) s on the m22 branch", None),
    "order_m11_m22": ("cm_quat_from_mat: the m11 branch taken when m22 > m11", None),
    "no_factor_2": ("to_rodrigues: angle = acos(q0)", None),
    "no_renorm": ("to_rodrigues: the axis not renormalised", "scaled"),
    "center_transpose": ("cm_center: the transpose instead of the inverse", "scaled"),
    "sin_sign": ("cm_from_axis_angle: o[1] = k ax ay - s az", None),
}


def _outside(f, mutation):
    """entries of family f that the mutated restatement puts outside C E (E of the arithmetic as it is)"""
    cam = f["cam15"]
    n = 0
    with np.errstate(all="ignore"):
        _, E, masks = R.to_vec(cam, rotation=f["rotation"])
        W = R.to_vec(cam, (mutation,), rotation=f["rotation"])[0]
        n += int(R.outside(W, _to_vec_reference(f, W, masks), E).sum())
        _, Ec = R.center(cam)
        c = R.center(cam, (mutation,))[0]
        res, scale = R.center_residual(cam, c)
        n += int((~(np.abs(res).astype(np.float64) <= J.C * R.center_bound(cam, Ec) + scale.astype(np.float64) * TWO60 + J.FLOOR)).sum())
        if f["bal9"] is not None:
            _, Er, _ = R.from_vec(f["bal9"])
            Rv = R.from_vec(f["bal9"], (mutation,))[0]
            n += int(R.outside(Rv, R.colmajor(J.exp_so3(f["bal9"][:, 0:3])), Er).sum())
    return n


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_mutations_fall_outside_the_bound(fams, mutation):
    what, where = MUTATIONS[mutation]
    n = {name: _outside(f, mutation) for name, f in fams.items()}
    print("[camref] %s (%s): entries outside C E per family %s" % (mutation, what, n))
    assert sum(n.values()) > 0, "%s (%s) stays inside C E everywhere" % (mutation, what)
    if where is not None:
        assert n[where] > 0, "%s (%s) stays inside C E on %s" % (mutation, what, where)


def test_unmutated_restatement_has_nothing_outside(fams):
    assert all(_outside(f, "none") == 0 for f in fams.values())
