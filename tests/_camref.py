"""Extended-precision reference and a running error bound for the camera conversions and the camera table (test helper;
shared by tests/test_camref.py and tests/test_gpu_camera_reference.py).

Three parts:
  * the reference in np.longdouble, in forms that do not follow the kernel: exp_so3 (tests/_jacref.py) for from_vec;
    log_ld for to_vec -- the quaternion from the LARGEST of its four candidates, the angle as 2 atan2(|v|, q0) in [0, pi],
    the axis as v / |v| -- returning the representative the device must produce (theta n, or (theta - 2 pi) n when the
    quantity the device's branch takes the sign of q0 from is negative); the centre is judged by its residual R c + t;
  * camera_math.hpp's cm_quat_from_mat, to_rodrigues and cm_center restated in numpy f64 in the kernel's order with
    _jacref.V beside every value (from_rodrigues is _jacref's).  The build uses -ffp-contract=off: every operation but
    sin, cos and acos is IEEE-exact, so the restated values are the device's bit for bit wherever no transcendental enters;
  * the families of cameras the tests draw.

A to_vec result passes when |w_dev - log_ld(R)| <= C E + |ref| 2^-60 + FLOOR (tolerance()).  E knows the curve of the
reference's formula angle = 2 acos(q0): the error of q0 (one rounding, ~1e-16) is divided by sin(theta / 2), and below
1 - q0^2 < f64::EPSILON (theta < 2 sqrt(eps) = 2.98e-8) exactly 0 is returned: the error is theta itself."""
import itertools

import numpy as np

import _jacref as J
from _jacref import LD, U, KEPS, FLOOR, V

# The device's f64 acos (ocml), in ulps of its result.  The ROCm documentation installed with the toolchain states no bound
# for it, so this is measured: over every family the device's to_vec lies within 1 ulp of the angle of
# the restatement whose acos is the long-double arccos rounded once (test_to_vec prints the figure); plus one ulp of margin.
ACOS_ULP = 2.0            # measured 1 + 1 (the project's TRIG_ULP = 1 for sin / cos was the starting point)

PI_LD = 4 * np.arctan(LD(1))


# ==================================================================================================================
# reference (longdouble)
# ==================================================================================================================
def rowmajor(Rcm):
    """[n, 9] column-major (cam15's order: m[3 c + r]) -> [n, 3, 3] R[n][r][c], same dtype"""
    return np.asarray(Rcm).reshape(-1, 3, 3).transpose(0, 2, 1)


def colmajor(R):
    return np.ascontiguousarray(np.asarray(R).transpose(0, 2, 1).reshape(-1, 9))


def defect(Rcm):
    """max |R^T R - I| per camera (longdouble -> f64): how far the matrix is from a rotation"""
    R = rowmajor(np.asarray(Rcm, dtype=LD))
    G = np.einsum("nki,nkj->nij", R, R) - np.eye(3, dtype=LD)
    return np.abs(G).reshape(len(R), 9).max(axis=1).astype(np.float64)


def branch_masks(Rcm):
    """cm_quat_from_mat's four branches on f64 matrices, decided as the device decides them (f64, its order of the sum)"""
    m = np.asarray(Rcm, dtype=np.float64)
    trace = (m[:, 0] + m[:, 4]) + m[:, 8]
    b0 = trace >= 0.0
    b1 = ~b0 & (m[:, 0] > m[:, 4]) & (m[:, 0] > m[:, 8])
    b2 = ~b0 & ~b1 & (m[:, 4] > m[:, 8])
    b3 = ~b0 & ~b1 & ~b2
    return b0, b1, b2, b3


def log_ld(Rcm, delta=None):
    """(w, other, either): w [n, 3] the rotation vector the device must produce for the f64 (or longdouble) matrices Rcm
    [n, 9]; `other` the representative 2 pi away along the axis; `either` where the sign that chooses between them is
    within its own rounding of 0 (theta = pi) and both are accepted."""
    R = rowmajor(np.asarray(Rcm, dtype=LD))
    n = len(R)
    d = R[:, [0, 1, 2], [0, 1, 2]]
    tr = d.sum(axis=1)
    cand = np.stack([1 + tr, 1 + d[:, 0] - d[:, 1] - d[:, 2], 1 - d[:, 0] + d[:, 1] - d[:, 2], 1 - d[:, 0] - d[:, 1] + d[:, 2]], axis=1)
    k = np.argmax(cand, axis=1)
    big = 2 * np.sqrt(cand[np.arange(n), k])                          # 4 |q_k|
    a = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)      # 4 q0 v
    s = np.stack([R[:, 0, 1] + R[:, 1, 0], R[:, 0, 2] + R[:, 2, 0], R[:, 1, 2] + R[:, 2, 1]], axis=1)      # 4 (xy, xz, yz)
    q = np.empty((n, 4), dtype=LD)
    quarter = big / 4
    forms = [(quarter, a[:, 0] / big, a[:, 1] / big, a[:, 2] / big),
             (a[:, 0] / big, quarter, s[:, 0] / big, s[:, 1] / big),
             (a[:, 1] / big, s[:, 0] / big, quarter, s[:, 2] / big),
             (a[:, 2] / big, s[:, 1] / big, s[:, 2] / big, quarter)]
    for j, f in enumerate(forms):
        sel = k == j
        for c in range(4):
            q[sel, c] = f[c][sel]
    q = np.where((q[:, 0] < 0)[:, None], -q, q)
    nv = np.sqrt((q[:, 1:] ** 2).sum(axis=1))
    theta = 2 * np.arctan2(nv, q[:, 0])
    axis = q[:, 1:] / np.where(nv > 0, nv, LD(1))[:, None]
    # the sign of the device's q0: + on the trace branch, the sign of the antisymmetric part it divides on the others
    b0, b1, b2, _ = branch_masks(np.asarray(Rcm, dtype=np.float64))
    sq = np.where(b0, LD(1), np.where(b1, a[:, 0], np.where(b2, a[:, 1], a[:, 2])))
    mag = np.where(b1, np.abs(R[:, 2, 1]) + np.abs(R[:, 1, 2]), np.where(b2, np.abs(R[:, 0, 2]) + np.abs(R[:, 2, 0]),
                                                                           np.abs(R[:, 1, 0]) + np.abs(R[:, 0, 1])))
    dl = 0 if delta is None else np.asarray(delta, dtype=LD)
    either = ~b0 & (np.abs(sq) <= 8 * U * mag + 2 * dl)
    plus, minus = theta[:, None] * axis, (theta - 2 * PI_LD)[:, None] * axis
    neg = (sq < 0)[:, None]
    return np.where(neg, minus, plus), np.where(neg, plus, minus), either


def nearest(dev, w, other, either):
    """the reference per camera: `other` where both representatives are accepted and it lies closer to dev"""
    dev = np.asarray(dev, dtype=LD)
    closer = np.abs(dev - other).max(axis=1) < np.abs(dev - w).max(axis=1)
    return np.where((either & closer)[:, None], other, w)


def center_residual(cam15, c):
    """R c + t in longdouble [n, 3], and the scale |R| |c| + |t| its rounding refers to"""
    m = np.asarray(cam15, dtype=LD)
    R, c = rowmajor(m[:, 0:9]), np.asarray(c, dtype=LD)
    return np.einsum("nij,nj->ni", R, c) + m[:, 9:12], np.einsum("nij,nj->ni", np.abs(R), np.abs(c)) + np.abs(m[:, 9:12])


# ==================================================================================================================
# the kernel's order in f64, with a running error bound
# ==================================================================================================================
def acos_once(x):
    """long-double arccos rounded once to f64 (NaN outside [-1, 1], like the device's)"""
    with np.errstate(invalid="ignore"):
        return np.arccos(np.asarray(x, dtype=np.float64).astype(LD)).astype(np.float64)


def vacos(x):
    """acos: the argument's error through the largest slope on [|x| - e, |x| + e], capped by acos's own modulus of
    continuity (|acos a - acos b| <= acos(1 - |a - b|)) where the slope blows up; its own error ACOS_ULP ulps"""
    v = acos_once(x.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        hi = np.minimum(np.abs(x.v) + x.e, 1.0)
        slope = np.where(x.e > 0, x.e / np.sqrt(1.0 - hi * hi), 0.0)
        cap = np.arccos(np.clip(1.0 - x.e, -1.0, 1.0))
    return V(v, np.minimum(slope, cap) + 2 * ACOS_ULP * U * np.abs(v))


class _OpsV:
    sqrt, acos, where = staticmethod(J.vsqrt), staticmethod(vacos), staticmethod(J.where)
    scale = staticmethod(lambda x, k: x.exact_scale(k))
    val = staticmethod(lambda x: x.v)


class _OpsLD:
    """the same expression tree evaluated in longdouble: what the FORMULA gives on a matrix that is no rotation"""
    sqrt, acos, where = staticmethod(np.sqrt), staticmethod(np.arccos), staticmethod(np.where)
    scale = staticmethod(lambda x, k: x * k)
    val = staticmethod(lambda x: x)


def quat_from_mat(m, ops=_OpsV, masks=None, mutations=()):
    """camera_math.hpp cm_quat_from_mat: m col-major (9 values), q = (w, x, y, z); the four branches through where"""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m
    trace = m00 + m11 + m22
    if masks is None:
        v = ops.val
        b0 = v(trace) >= 0.0
        b1 = ~b0 & (v(m00) > v(m11)) & (v(m00) > v(m22))
        b2 = ~b0 & ~b1 & ((v(m22) > v(m11)) if "order_m11_m22" in mutations else (v(m11) > v(m22)))
        masks = (b0, b1, b2)
    b0, b1, b2 = masks
    flip = ["sign_b%d" % k in mutations for k in (1, 2, 3)]             # one sum of a non-trace branch turned into a difference
    with np.errstate(all="ignore"):
        s = ops.sqrt(1.0 + trace)
        w0, s = ops.scale(s, 0.5), 0.5 / s
        q0 = (w0, (m12 - m21) * s, (m20 - m02) * s, (m01 - m10) * s)
        s = ops.sqrt((m00 - m11 - m22) + 1.0)
        x1, s = ops.scale(s, 0.5), 0.5 / s
        q1 = ((m12 - m21) * s, x1, ((m10 - m01) if flip[0] else (m10 + m01)) * s, (m02 + m20) * s)
        s = ops.sqrt((m11 - m00 - m22) + 1.0)
        y2, s = ops.scale(s, 0.5), 0.5 / s
        q2 = ((m20 - m02) * s, (m10 + m01) * s, y2, ((m21 - m12) if flip[1] else (m21 + m12)) * s)
        s = ops.sqrt((m22 - m00 - m11) + 1.0)
        z3, s = ops.scale(s, 0.5), 0.5 / s
        q3 = ((m01 - m10) * s, ((m02 - m20) if flip[2] else (m02 + m20)) * s, (m21 + m12) * s, z3)
    return [ops.where(b0, q0[k], ops.where(b1, q1[k], ops.where(b2, q2[k], q3[k]))) for k in range(4)], masks


def to_rodrigues(m, ops=_OpsV, masks=None, mutations=()):
    """camera_math.hpp to_rodrigues on col-major m (9 values): (w list of 3, masks = (b0, b1, b2, zero))"""
    q, bm = quat_from_mat(m, ops, None if masks is None else masks[:3], mutations)
    with np.errstate(all="ignore"):
        ac = ops.acos(q[0])
        angle = ac if "no_factor_2" in mutations else ops.scale(ac, 2.0)
        one_m = 1.0 - q[0] * q[0]
        zero = (ops.val(one_m) < (1e-8 if "to_cutoff" in mutations else KEPS)) if masks is None else masks[3]
        d = ops.sqrt(one_m)
        if ops is _OpsV:
            # the renormalisation below makes the axis (q.xyz / d) / |q.xyz / d| independent of d in exact arithmetic: the bound
            # takes the rounded d as that arbitrary scale (no input error), so that the error of 1 - q0^2 -- relative error
            # of order one next to the cut-off -- is not charged to a result it cannot reach
            d = V(d.v)
        ax, ay, az = q[1] / d, q[2] / d, q[3] / d
        inv = 1.0 if "no_renorm" in mutations else 1.0 / ops.sqrt(J.dot3((ax, ay, az), (ax, ay, az)))
        w = [(ax * inv) * angle, (ay * inv) * angle, (az * inv) * angle]
    if ops is _OpsV:
        # the cut-off returns exactly 0 for an angle of up to 2 asin(sqrt(eps + what one_m may be off by)): the error is the angle
        ez = 2 * np.arcsin(np.sqrt(np.clip(KEPS + one_m.e, 0.0, 1.0))) * (1 + 1e-6)
        z = V(np.zeros_like(one_m.v), ez)
        w = [J.where(zero, z, x) for x in w]
    else:
        w = [np.where(zero, LD(0), x) for x in w]
    return w, bm + (zero,)


REF_SENS = 8.0      # |log_ld(M) - log(R*)| <= REF_SENS delta for M within delta of the rotation R* (see to_vec)


def to_vec(cam15, mutations=(), rotation=True, R_err=None):
    """cameras_to_bal's rotation part restated: (W [n, 3] values, E [n, 3], masks).  With rotation=True the matrix is read
    as a rotation known to within its own distance from one (delta = max |R^T R - I|, or R_err [n, 9] where the caller knows
    the entries' bound): every entry carries that as its input error, and E gains REF_SENS delta for the reference -- the
    quaternion of the largest candidate moves by at most 3 delta under such a change of the matrix (|q_k| >= 1 / 2), and
    theta n = 2 atan2(|v|, q0) v / |v| by at most twice that plus the axis term 2 |dv|.  With rotation=False the entries are
    exact and E bounds the distance from the formula itself (formula_ld)."""
    c = np.asarray(cam15, dtype=np.float64)
    n = len(c)
    if R_err is not None:
        e9 = np.asarray(R_err, dtype=np.float64)
        dl = e9.max(axis=1) if n else np.zeros(0)
    else:
        dl = defect(c[:, 0:9]) if rotation else np.zeros(n)
        e9 = np.broadcast_to(dl[:, None], (n, 9))
    w, masks = to_rodrigues([V(c[:, k], e9[:, k]) for k in range(9)], mutations=mutations)
    W = np.stack([x.v for x in w], axis=1)
    E = np.stack([x.e for x in w], axis=1) + REF_SENS * dl[:, None]
    return W, E, masks


def formula_ld(cam15, masks):
    """to_rodrigues' own expression tree in longdouble on the branches the f64 run took [n, 3]"""
    c = np.asarray(cam15, dtype=LD)
    w, _ = to_rodrigues([c[:, k] for k in range(9)], ops=_OpsLD, masks=masks)
    return np.stack(w, axis=1)


def from_vec(bal9, mutations=()):
    """cameras_from_bal's rotation restated (_jacref.from_rodrigues): (R col-major values [n, 9], E [n, 9], small [n]) --
    small = the branch without sin / cos (theta^2 <= f64::EPSILON), where the values are the device's bits"""
    b = np.asarray(bal9, dtype=np.float64)
    w = [V(b[:, k]) for k in range(3)]
    with np.errstate(all="ignore"):
        R = J.from_rodrigues(*w, mutations=mutations)
        theta2 = J.dot3(w, w).v
    small = ~(theta2 > (1e-8 if "rodrigues_threshold" in mutations else KEPS))
    if "sin_sign" in mutations:                                       # o[1] = k ax ay - s az: the expression of o[3]
        R[1] = J.where(~small, R[3], R[1])
    return np.stack([x.v for x in R], axis=1), np.stack([x.e for x in R], axis=1), small


def center(cam15, mutations=()):
    """camera_math.hpp cm_center restated: (c [n, 3] values, E [n, 3]); the matrix and t are exact inputs"""
    c = np.asarray(cam15, dtype=np.float64)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (V(c[:, k]) for k in range(9))
    t = [V(c[:, 9 + k]) for k in range(3)]
    if "center_transpose" in mutations:
        rows = [(m00, m01, m02), (m10, m11, m12), (m20, m21, m22)]
    else:
        det = m00 * (m11 * m22 - m21 * m12) - m10 * (m01 * m22 - m21 * m02) + m20 * (m01 * m12 - m11 * m02)
        rows = [((m11 * m22 - m12 * m21) / det, (m12 * m20 - m10 * m22) / det, (m10 * m21 - m11 * m20) / det),
                ((m21 * m02 - m22 * m01) / det, (m22 * m00 - m20 * m02) / det, (m20 * m01 - m21 * m00) / det),
                ((m01 * m12 - m02 * m11) / det, (m02 * m10 - m00 * m12) / det, (m00 * m11 - m01 * m10) / det)]
    out = [-J.dot3(r, t) for r in rows]
    return np.stack([x.v for x in out], axis=1), np.stack([x.e for x in out], axis=1)


def center_bound(cam15, Ec):
    """what a centre within Ec of -R^-1 t leaves of R c + t: |R| Ec, row by row"""
    return np.einsum("nij,nj->ni", np.abs(rowmajor(np.asarray(cam15, dtype=np.float64)[:, 0:9])), Ec)


def exp_bound(Ew, dl):
    """bound on the entries of exp(w') - R for |w' - log R| <= Ew: a rotation moves by at most sqrt(2) |dw| in Frobenius
    norm, and R itself is within dl of the rotation whose logarithm is meant"""
    return (np.sqrt(2.0) * np.sqrt((Ew * Ew).sum(axis=1)) + dl)[:, None] * np.ones((1, 9))


tolerance, ratio = J.tolerance, J.ratio


def outside(dev, ref, E):
    """entries outside C E (a NaN is outside)"""
    err = np.abs(np.asarray(dev, dtype=LD) - ref).astype(np.float64)
    return ~(err <= tolerance(E, ref))


def sharp_tolerance(W):
    """device against restatement, the same IEEE operations on the same bits but for acos: ACOS_ULP ulps of the angle (one
    ulp <= 2 u |value|), carried into each component, plus the rounding of the last product on either side"""
    return 2 * ACOS_ULP * U * np.abs(W) + 2 * U * np.abs(W) + FLOOR


# ==================================================================================================================
# families
# ==================================================================================================================
_S = np.sqrt(KEPS)                                                    # 2^-26: its square is f64::EPSILON exactly
ANGLES = (0.0, 1e-300, 1e-160, 1e-9, np.nextafter(_S, 0.0), _S, np.nextafter(_S, 1.0), 2.9e-8, 3.1e-8, 1e-7, 1e-6, 1e-4, 1e-2,
          0.1, 1.0, np.pi / 2, 2 * np.pi / 3, np.pi - 1e-8, np.pi, np.pi + 1e-8, 4.0, 5.0, 2 * np.pi - 1e-6, 2 * np.pi - 1e-9,
          2 * np.pi, 7.0, 100.0)
ANGLE_NAMES = ("0", "1e-300", "1e-160", "1e-9", "sqrt(eps)-", "sqrt(eps)", "sqrt(eps)+", "2.9e-8", "3.1e-8", "1e-7", "1e-6", "1e-4",
               "1e-2", "0.1", "1", "pi/2", "2pi/3", "pi-1e-8", "pi", "pi+1e-8", "4", "5", "2pi-1e-6", "2pi-1e-9", "2pi", "7", "100")
N_RANDOM_AXES = 8
FIXED_AXES = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [np.sqrt(0.5), np.sqrt(0.5), 0], [np.sqrt(1 / 3.0)] * 3])
FAMILIES = ("angles", "cube", "branches", "drifted", "scaled")
ROTATION_FAMILIES = ("angles", "cube", "branches", "drifted")


def _translations(rng, n):
    return 10.0 ** rng.uniform(-3, 6, size=(n, 3)) * np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0)


def _intrinsics(rng, n):
    f = 10.0 ** rng.uniform(-0.3, 3.5, n)
    k = rng.normal(size=(n, 2)) * 10.0 ** rng.uniform(-6, 0, size=(n, 2))
    k[::7, 1] = np.array([0.0, -0.0, 5e-324, -5e-324])[np.arange(len(k[::7])) % 4]
    return np.column_stack([f, k])


def _cam15(R, rng):
    """[n, 3, 3] row-major rotations (any dtype) -> cam15 with the family's translations and intrinsics"""
    R = np.asarray(R)
    return np.ascontiguousarray(np.column_stack([colmajor(R).astype(np.float64), _translations(rng, len(R)), _intrinsics(rng, len(R))]))


def _exp(w):
    """exp(w) rounded once from longdouble [n, 3, 3] f64"""
    return J.exp_so3(np.asarray(w, dtype=np.float64)).astype(np.float64)


def family(name, seed=0):
    """dict(name, cam15 [n, 15], bal9 [n, 9] or None, label [n] of str, rotation): see the module's families
      angles    |w| at every branch point of from_vec and to_vec (ANGLES) on 8 random axes, the coordinate axes, (1,1,0)/sqrt 2
                and (1,1,1)/sqrt 3; bal9 = the vectors, cam15 = exp(w) rounded once from longdouble;
      cube      the 24 proper rotations with entries 0 and +-1 (120 degrees: trace exactly 0; 180 degrees: trace -1 and every tie
                of m00 > m11, m11 > m22; the identity: the zero branch) and the generators' directions as tests/_problems.py
                builds them, eight translations each;
      branches  theta in [pi - 0.3, pi + 0.3] about axes dominated by x, y and z in turn (the three branches without the
                trace), and theta in [2 pi / 3 - 0.3, 2 pi / 3 + 0.3] about any axis (either side of trace = 0);
      drifted   rotations times 50 small rotations in f64: ~1e-14 from orthonormal;
      scaled    rotations times 1 +- 1e-6 and general matrices with determinant in [0.5, 2]: no rotations."""
    rng = np.random.default_rng(1000 + seed)
    bal9 = None
    if name == "angles":
        per = N_RANDOM_AXES + len(FIXED_AXES)
        mag = np.repeat(np.array(ANGLES), per)
        ax = np.concatenate([np.concatenate([J._unit(rng, N_RANDOM_AXES), FIXED_AXES]) for _ in ANGLES])
        w = ax * mag[:, None]
        cam15 = _cam15(_exp(w), rng)
        bal9 = np.ascontiguousarray(np.column_stack([w, cam15[:, 9:15]]))
        label = np.repeat(np.array(ANGLE_NAMES, dtype=object), per)
    elif name == "cube":
        import oracle as O
        mats, labs = [], []
        for perm in itertools.permutations(range(3)):
            for sg in itertools.product((1.0, -1.0), repeat=3):
                M = np.zeros((3, 3))
                for r in range(3):
                    M[r, perm[r]] = sg[r]
                if round(np.linalg.det(M)) == 1:
                    mats.append(M)
                    labs.append("cube/%d" % {3: 0, 1: 90, 0: 120, -1: 180}[int(np.trace(M))])
        gen = {"gen/-90": O.basis_from_angle_y_deg(-90.0), "gen/90": O.basis_from_angle_y_deg(90.0),
               "gen/180": O.basis_from_angle_y_deg(180.0), "gen/one": np.array([1, 0, 0, 0, 1, 0, 0, 0, 1.0])}
        for key, cm in gen.items():
            mats.append(rowmajor(cm[None, :])[0])
            labs.append(key)
        assert len(mats) == 28
        cam15 = _cam15(np.tile(np.array(mats), (8, 1, 1)), rng)
        label = np.array(labs * 8, dtype=object)
    elif name == "branches":
        m = 300
        axes, th, label = [], [], []
        for k, key in enumerate(("x", "y", "z")):
            a = 0.45 * rng.normal(size=(m, 3))
            a[:, k] = np.where(rng.random(m) < 0.5, -1.0, 1.0)
            axes.append(a / np.linalg.norm(a, axis=1, keepdims=True))
            th.append(np.pi + rng.uniform(-0.3, 0.3, m))
            label += ["pi/" + key] * m
        axes.append(J._unit(rng, m))
        th.append(2 * np.pi / 3 + rng.uniform(-0.3, 0.3, m))
        label += ["2pi/3"] * m
        cam15 = _cam15(_exp(np.concatenate(axes) * np.concatenate(th)[:, None]), rng)
        label = np.array(label, dtype=object)
    elif name == "drifted":
        m = 300
        R = _exp(J._unit(rng, m) * (10.0 ** rng.uniform(-5, np.log10(3.0), m))[:, None])
        for _ in range(50):
            R = np.einsum("nij,njk->nik", R, _exp(1e-3 * rng.normal(size=(m, 3))))
        cam15 = _cam15(R, rng)
        label = np.full(m, "drifted", dtype=object)
    elif name == "scaled":
        m, g = 260, 40
        R = _exp(J._unit(rng, m + g) * (10.0 ** rng.uniform(-5, np.log10(3.0), m + g))[:, None])
        sc = np.where(np.arange(m) % 2 == 0, 1 + 1e-6, 1 - 1e-6)
        R[:m] *= sc[:, None, None]
        G = np.einsum("nij,njk->nik", R[m:], np.eye(3) + 0.15 * rng.normal(size=(g, 3, 3)))
        det = np.linalg.det(G)
        bad = (det < 0.5) | (det > 2.0)
        G[bad] *= (np.cbrt(1.0 / np.abs(det[bad])) * np.sign(det[bad]))[:, None, None]
        det = np.linalg.det(G)
        assert np.all((det >= 0.5) & (det <= 2.0)), det
        R[m:] = G
        cam15 = _cam15(R, rng)
        label = np.array(["scaled/1+1e-6" if s > 1 else "scaled/1-1e-6" for s in sc] + ["scaled/general"] * g, dtype=object)
    else:
        raise AssertionError(name)
    cam15.setflags(write=False)
    return dict(name=name, cam15=cam15, bal9=bal9, label=label, rotation=name in ROTATION_FAMILIES)


_cache = {}


def families():
    """every family once (cached, read-only)"""
    if not _cache:
        for k, name in enumerate(FAMILIES):
            _cache[name] = family(name, seed=k)
        assert sum(len(f["cam15"]) for f in _cache.values()) < 20_000
    return _cache


def bal9_of(f):
    """a family's 9-vectors: its own where it has them, the restated to_vec of its matrices otherwise"""
    if f["bal9"] is not None:
        return f["bal9"]
    return np.ascontiguousarray(np.column_stack([to_vec(f["cam15"], rotation=False)[0], f["cam15"][:, 9:15]]))


POOL = 1025
POOL_COUNTS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1025)


def pool():
    """(cam15 [1025, 15], bal9 [1025, 9]) drawn from all families: the count-edge tests' cameras.  The 9-vectors of the
    families given as matrices are their restated to_vec."""
    F = families()
    cam = np.concatenate([F[k]["cam15"] for k in FAMILIES])
    bal = np.concatenate([bal9_of(F[k]) for k in FAMILIES])
    pick = np.random.default_rng(77).permutation(len(cam))[:POOL]
    return np.ascontiguousarray(cam[pick]), np.ascontiguousarray(bal[pick])
