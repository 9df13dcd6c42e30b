"""Extended-precision reference for the reprojection Jacobian, and a running error bound for the kernel's order of
operations (test helper; shared by tests/test_jacobian_reference.py and tests/test_gpu_jacobian_entries.py).

Two halves:
  * reference_bal / reference_state: r, Jc [n,2,9] (to_vec columns w t f k1 k2) and Jp [n,2,3] in np.longdouble (x87
    80-bit: 64-bit mantissa, 11 bits beyond f64), from forms that do not follow the kernel's:
      bal mode   -- R = exp(w) of the 9-vector's own w; the rotation columns are the exact directional derivative of
                    Rodrigues' formula R = I + A K + B K^2 (K = [w]x), with series for A, B and their derivatives below
                    |w| = 2;
      state mode -- the kernel's definition: the left perturbation at the stored R (cam15) mapped through J_l(w), w being
                    the device's to_vec of that R.
    Both take |p|^4 the way the reference has it: rad = 1 + k1 n + k2 |p|^4 (= n^2 exactly), d rad / d n = k1 + 2 k2 n.
  * kernel_f64: the device arithmetic of camera_math.hpp (from_rodrigues in bal mode, left_jacobian, project_head /
    project_tail) and kernels.hpp (jacobian_obs) restated in numpy f64 in the kernel's order -- FMAs through longdouble --
    carrying beside every value a first-order running error bound: each rounded operation adds u |result| (an FMA counts
    once), the device's sin / cos and libm's pow add one ulp, the two series of left_jacobian and the small-angle branch of
    from_rodrigues add their truncation.  E therefore bounds |kernel - exact| for the KERNEL's grouping.

A kernel entry passes when |J_dev - J_ref| <= C E + |J_ref| 2^-60 + FLOOR (tolerance()).  `mutations` switches one-line
changes of the kernel on in the restatement (tests/test_jacobian_reference.py shows that each lands outside the bound)."""
import numpy as np

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise RuntimeError("tests/_jacref.py needs an extended long double (64-bit mantissa, x87 80-bit); this platform's "
                       "np.longdouble has %d mantissa bits -- the reference would be no better than the kernel it judges"
                       % np.finfo(LD).nmant)

U = 2.0 ** -53            # unit roundoff of f64
C = 4.0                   # tolerance = C * E: E is a worst-case first-order bound, C its margin against second-order terms
FLOOR = 4 * 5e-324        # a few subnormals: results that underflow round absolutely
KEPS = 2.220446049250313e-16
TRIG_ULP = 1.0            # device sin / cos (ocml), glibc pow: within one ulp (one ulp <= 2u |result|)

COLS = ("w0", "w1", "w2", "t0", "t1", "t2", "f", "k1", "k2")
PCOLS = ("X", "Y", "Z")


# ==================================================================================================================
# reference (longdouble)
# ==================================================================================================================
def _series(x, coef):
    """sum_k coef[k] x^k (Horner, longdouble)"""
    acc = np.zeros_like(x)
    for cf in reversed(coef):
        acc = acc * x + cf
    return acc


def _fact(k):
    out = LD(1)
    for i in range(2, k + 1):
        out *= LD(i)
    return out


_NS = 32
_A = [LD((-1) ** k) / _fact(2 * k + 1) for k in range(_NS)]                       # sin t / t
_B = [LD((-1) ** k) / _fact(2 * k + 2) for k in range(_NS)]                       # (1 - cos t) / t^2
_Cb = [LD((-1) ** k) / _fact(2 * k + 3) for k in range(_NS)]                      # (t - sin t) / t^3
_dA = [LD((-1) ** (k + 1)) * (2 * k + 2) / _fact(2 * k + 3) for k in range(_NS)]  # A'(t) / t
_dB = [LD((-1) ** (k + 1)) * (2 * k + 2) / _fact(2 * k + 4) for k in range(_NS)]  # B'(t) / t


def rodrigues_coeffs(th2):
    """A = sin t / t, B = (1 - cos t) / t^2, Cb = (t - sin t) / t^3, dA = A'(t) / t, dB = B'(t) / t for t^2 = th2 (longdouble):
    series below t = 2 (all terms of one sign pattern and decreasing: no cancellation), closed forms above."""
    th2 = np.asarray(th2, dtype=LD)
    small = th2 < 4
    A, B, Cb, dA, dB = (_series(th2, c) for c in (_A, _B, _Cb, _dA, _dB))
    if not np.all(small):
        tb = np.where(small, LD(3), th2)
        t = np.sqrt(tb)
        s, c = np.sin(t), np.cos(t)
        A = np.where(small, A, s / t)
        B = np.where(small, B, (1 - c) / tb)
        Cb = np.where(small, Cb, (t - s) / (tb * t))
        dA = np.where(small, dA, (t * c - s) / (tb * t))
        dB = np.where(small, dB, (t * s - 2 * (1 - c)) / (tb * tb))
    return A, B, Cb, dA, dB


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _image(q, intr, Dq):
    """uv and the blocks from the camera-frame point q [n,3] and dq/d(rotation) Dq [n,3,3]; intr = (f, k1, k2)"""
    f, k1, k2 = intr[:, 0], intr[:, 1], intr[:, 2]
    px, py = -q[:, 0] / q[:, 2], -q[:, 1] / q[:, 2]
    n = px * px + py * py
    rad = 1 + k1 * n + k2 * (n * n)
    c = 2 * k1 + 4 * k2 * n                                   # 2 d rad / d n
    p = np.stack([px, py], axis=1)
    # d p / d q = [[-1/z, 0, -px/z], [0, -1/z, -py/z]];  d (rad p) / d p = rad I + c p p^T
    iz = -1 / q[:, 2]
    dpdq = np.zeros(q.shape[:1] + (2, 3), dtype=LD)
    dpdq[:, 0, 0] = iz
    dpdq[:, 1, 1] = iz
    dpdq[:, 0, 2] = px * iz
    dpdq[:, 1, 2] = py * iz
    M = rad[:, None, None] * np.eye(2, dtype=LD) + c[:, None, None] * p[:, :, None] * p[:, None, :]
    A = f[:, None, None] * np.einsum("nij,njk->nik", M, dpdq)           # d uv / d q  [n,2,3]
    Jc = np.zeros(q.shape[:1] + (2, 9), dtype=LD)
    Jc[:, :, 0:3] = np.einsum("nij,njk->nik", A, Dq)
    Jc[:, :, 3:6] = A
    Jc[:, :, 6] = rad[:, None] * p
    Jc[:, :, 7] = (f * n)[:, None] * p
    Jc[:, :, 8] = (f * n * n)[:, None] * p
    uv = (f * rad)[:, None] * p
    return uv, Jc, A, p


def exp_so3(w):
    """exp([w]x) [n,3,3] (longdouble)"""
    w = np.asarray(w, dtype=LD)
    A, B = rodrigues_coeffs(_dot(w, w))[:2]
    K = np.zeros(w.shape[:1] + (3, 3), dtype=LD)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -w[:, 2], w[:, 1], -w[:, 0]
    K[:, 1, 0], K[:, 2, 0], K[:, 2, 1] = w[:, 2], -w[:, 1], w[:, 0]
    return np.eye(3, dtype=LD) + A[:, None, None] * K + B[:, None, None] * np.einsum("nij,njk->nik", K, K)


def left_jacobian_ld(w):
    """J_l(w) = I + B K + Cb K^2 [n,3,3] (longdouble)"""
    w = np.asarray(w, dtype=LD)
    _, B, Cb, _, _ = rodrigues_coeffs(_dot(w, w))
    K = np.zeros(w.shape[:1] + (3, 3), dtype=LD)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -w[:, 2], w[:, 1], -w[:, 0]
    K[:, 1, 0], K[:, 2, 0], K[:, 2, 1] = w[:, 2], -w[:, 1], w[:, 0]
    return np.eye(3, dtype=LD) + B[:, None, None] * K + Cb[:, None, None] * np.einsum("nij,njk->nik", K, K)


def reference_bal(bal9, X, uv_obs=None):
    """bal mode: camera = the 9-vector (w t f k1 k2), R = exp(w).  Returns dict(r, uv, Jc, Jp, q) in longdouble."""
    b = np.asarray(bal9, dtype=LD)
    X = np.asarray(X, dtype=LD)
    w, t, intr = b[:, 0:3], b[:, 3:6], b[:, 6:9]
    A, B, _, dA, dB = rodrigues_coeffs(_dot(w, w))
    wx, wX = _cross(w, X), _dot(w, X)
    K2X = w * wX[:, None] - _dot(w, w)[:, None] * X
    q = X + A[:, None] * wx + B[:, None] * K2X + t
    # d(RX)/dw_j = dA w_j (w x X) + A (e_j x X) + dB w_j K^2 X + B (e_j (w.X) + w X_j - 2 w_j X)
    Dq = np.empty(X.shape[:1] + (3, 3), dtype=LD)
    E = np.eye(3, dtype=LD)
    for j in range(3):
        ej = np.broadcast_to(E[j], X.shape)
        Dq[:, :, j] = ((dA * w[:, j])[:, None] * wx + A[:, None] * _cross(ej, X) + (dB * w[:, j])[:, None] * K2X
                       + B[:, None] * (ej * wX[:, None] + w * X[:, j:j + 1] - 2 * w[:, j:j + 1] * X))
    uv, Jc, Aq, _ = _image(q, intr, Dq)
    Jp = np.einsum("nij,njk->nik", Aq, exp_so3(w))
    r = uv - (0 if uv_obs is None else np.asarray(uv_obs, dtype=LD))
    return dict(r=r, uv=uv, Jc=Jc, Jp=Jp, q=q)


def reference_state(cam15, w, X, uv_obs=None):
    """state mode: camera = cam15 (col-major R, t, f k1 k2) with rotation columns -[R X]x J_l(w) (w = to_vec of R as the
    device reports it).  Returns dict(r, uv, Jc, Jp, q) in longdouble."""
    c = np.asarray(cam15, dtype=LD)
    X = np.asarray(X, dtype=LD)
    R = c[:, 0:9].reshape(-1, 3, 3).transpose(0, 2, 1)                 # row-major [n][r][c]
    y = np.einsum("nij,nj->ni", R, X)
    q = y + c[:, 9:12]
    Jl = left_jacobian_ld(w)
    Dq = np.empty(X.shape[:1] + (3, 3), dtype=LD)
    for j in range(3):
        Dq[:, :, j] = _cross(Jl[:, :, j], y)                           # d q / d theta_j = (J_l e_j) x y
    uv, Jc, Aq, _ = _image(q, c[:, 12:15], Dq)
    Jp = np.einsum("nij,njk->nik", Aq, R)
    r = uv - (0 if uv_obs is None else np.asarray(uv_obs, dtype=LD))
    return dict(r=r, uv=uv, Jc=Jc, Jp=Jp, q=q)


# ==================================================================================================================
# the kernel's order in f64, with a running error bound
# ==================================================================================================================
class V:
    """value (f64, the kernel's rounding) and E >= |value - exact|, elementwise"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=np.float64)

    def __add__(self, o):
        o = _v(o)
        v = self.v + o.v
        return V(v, self.e + o.e + U * np.abs(v))

    def __sub__(self, o):
        o = _v(o)
        v = self.v - o.v
        return V(v, self.e + o.e + U * np.abs(v))

    def __rsub__(self, o):
        return _v(o) - self

    def __radd__(self, o):
        return _v(o) + self

    def __mul__(self, o):
        o = _v(o)
        v = self.v * o.v
        return V(v, np.abs(o.v) * self.e + np.abs(self.v) * o.e + self.e * o.e + U * np.abs(v))

    def __rmul__(self, o):
        return _v(o) * self

    def __truediv__(self, o):
        o = _v(o)
        v = self.v / o.v
        d = np.abs(o.v)
        rel = np.minimum(o.e / d, 0.5)
        return V(v, (self.e + np.abs(v) * o.e) / (d * (1 - rel)) + U * np.abs(v))

    def __rtruediv__(self, o):
        return _v(o) / self

    def __neg__(self):
        return V(-self.v, self.e)

    def exact_scale(self, k):
        """times a power of two: exact"""
        return V(self.v * k, self.e * abs(k))


def _v(x):
    return x if isinstance(x, V) else V(np.float64(x))


def const(c):
    """a decimal constant the compiler rounds to f64 (e.g. -1.0 / 24): its own rounding is an error against the exact value"""
    return V(np.float64(c), U * abs(float(c)))


def fma(a, b, c):
    a, b, c = _v(a), _v(b), _v(c)
    v = (a.v.astype(LD) * b.v.astype(LD) + c.v.astype(LD)).astype(np.float64)
    return V(v, np.abs(b.v) * a.e + np.abs(a.v) * b.e + a.e * b.e + c.e + U * np.abs(v))


def vsqrt(x):
    v = np.sqrt(x.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        prop = np.where(v > 0, x.e / (2 * np.where(v > 0, v, 1.0)), np.sqrt(x.e))
    return V(v, prop + U * v)


def vsin(x):
    v = np.sin(x.v)
    return V(v, np.abs(np.cos(x.v)) * x.e + 0.5 * x.e * x.e + 2 * TRIG_ULP * U * np.abs(v))


def vcos(x):
    v = np.cos(x.v)
    return V(v, np.abs(np.sin(x.v)) * x.e + 0.5 * x.e * x.e + 2 * TRIG_ULP * U * np.abs(v))


def vpow4(x):
    """libm's pow(x, 4.0) (pow4_libm): one ulp"""
    v = (x.v.astype(LD) ** 4).astype(np.float64)
    a = np.abs(x.v)
    return V(v, 4 * a ** 3 * x.e + 6 * a * a * x.e * x.e + 2 * TRIG_ULP * U * np.abs(v))


def vrcp(y):
    """1 / y by v_rcp_f64 + two Newton steps (jacobian_obs' iz): the estimate's error is squared twice (e^4, far below u
    for any estimate better than 2^-14) and the last step's rounding is one u"""
    v = 1.0 / y.v
    d = np.abs(y.v)
    return V(v, np.abs(v) * np.minimum(y.e / d, 0.5) / (1 - np.minimum(y.e / d, 0.5)) + 1.0001 * U * np.abs(v))


def where(cond, a, b):
    a, b = _v(a), _v(b)
    return V(np.where(cond, a.v, b.v), np.where(cond, a.e, b.e))


def dot3(a, b):
    """(a0 b0 + a1 b1) + a2 b2, separate roundings (-ffp-contract=off)"""
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def from_rodrigues(w0, w1, w2, mutations=()):
    """camera_math.hpp from_rodrigues: R col-major (list of 9 V)"""
    theta2 = dot3((w0, w1, w2), (w0, w1, w2))
    thr = 1e-8 if "rodrigues_threshold" in mutations else KEPS
    big = theta2.v > thr
    # axis-angle branch (cm_from_axis_angle)
    safe = V(np.where(big, theta2.v, 1.0), np.where(big, theta2.e, 0.0))
    angle = vsqrt(safe)
    inv = 1.0 / angle
    ax, ay, az = w0 * inv, w1 * inv, w2 * inv
    s, c = vsin(angle), vcos(angle)
    k = 1.0 - c
    o = [k * ax * ax + c, k * ax * ay + s * az, k * ax * az - s * ay,
         k * ax * ay - s * az, k * ay * ay + c, k * ay * az + s * ax,
         k * ax * az + s * ay, k * ay * az - s * ax, k * az * az + c]
    # small branch: cm_quat_from_mat of I + [w]x (trace 3: s = 2, q = (1, w / 2), all exact) then cm_mat_from_quat.  It is
    # R = I + K + K^2 / 2, whose truncation against exp is (A - 1) K + (B - 1/2) K^2: <= t^3 / 6 + t^4 / 24 per entry
    x, y, z = w0.exact_scale(0.5), w1.exact_scale(0.5), w2.exact_scale(0.5)
    x2, y2, z2 = x + x, y + y, z + z
    xx2, xy2, xz2 = x2 * x, x2 * y, x2 * z
    yy2, yz2, zz2 = y2 * y, y2 * z, z2 * z
    sy2, sz2, sx2 = y2 * 1.0, z2 * 1.0, x2 * 1.0
    m = [1.0 - yy2 - zz2, xy2 + sz2, xz2 - sy2,
         xy2 - sz2, 1.0 - xx2 - zz2, yz2 + sx2,
         xz2 + sy2, yz2 - sx2, 1.0 - xx2 - yy2]
    th = np.sqrt(np.abs(theta2.v) + theta2.e)
    trunc = th ** 3 / 6 + th ** 4 / 24
    m = [V(mi.v, mi.e + trunc) for mi in m]
    return [where(big, a, b) for a, b in zip(o, m)]


def left_jacobian(w0, w1, w2, mutations=()):
    """camera_math.hpp left_jacobian: J_l row-major (list of 9 V)"""
    t2 = (w0 * w0 + w1 * w1) + w2 * w2
    lim = 1e-1 if "series_1e-1" in mutations else 1e-2
    ser = t2.v < lim
    if "a_series_short" in mutations:                                   # the series of a cut after its t2^2 term
        a_s = const(0.5) + t2 * (const(-1.0 / 24) + t2 * const(1.0 / 720))
    else:
        a_s = const(0.5) + t2 * (const(-1.0 / 24) + t2 * (const(1.0 / 720) + t2 * (const(-1.0 / 40320) + t2 * const(1.0 / 3628800))))
    b_s = const(1.0 / 6) + t2 * (const(-1.0 / 120) + t2 * (const(1.0 / 5040) + t2 * (const(-1.0 / 362880) + t2 * const(1.0 / 39916800))))
    # truncation of the alternating series at the kernel's own switch (t2 < 1e-2): the first omitted term
    t2b = np.abs(t2.v) + t2.e
    a_s = V(a_s.v, a_s.e + np.where(t2b < 1e-2, t2b ** 5 / 479001600.0, 0.0))
    b_s = V(b_s.v, b_s.e + np.where(t2b < 1e-2, t2b ** 5 / 1307674368000.0, 0.0))
    safe = V(np.where(ser, 1.0, t2.v), np.where(ser, 0.0, t2.e))
    t = vsqrt(safe)
    sh = vsin(t.exact_scale(0.5))
    s = vsin(t)
    a_c = sh.exact_scale(2.0) * sh / safe
    b_c = (t - s) / (safe * t)
    a, b = where(ser, a_s, a_c), where(ser, b_s, b_c)
    return [1.0 + b * (w0 * w0 - t2), -a * w2 + b * w0 * w1, a * w1 + b * w0 * w2,
            a * w2 + b * w0 * w1, 1.0 + b * (w1 * w1 - t2), -a * w0 + b * w1 * w2,
            -a * w1 + b * w0 * w2, a * w0 + b * w1 * w2, 1.0 + b * (w2 * w2 - t2)]


def kernel_f64(mode, cams, X, w=None, mutations=()):
    """jacobian_obs restated.  mode "bal": cams = bal9 [n,9] (R = from_rodrigues(w), J_l(w) of the same w); mode "state":
    cams = cam15 [n,15] and w = to_vec [n,3].  Returns (Jc, Jp) as lists of V: Jc[i][j] i = 0,1 (u, v), j = 0..8."""
    cams = np.asarray(cams, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    if mode == "bal":
        w0, w1, w2 = (V(cams[:, k]) for k in range(3))
        Rcm = from_rodrigues(w0, w1, w2, mutations)
        t = [V(cams[:, 3 + k]) for k in range(3)]
        f, k1, k2 = (V(cams[:, 6 + k]) for k in range(3))
    else:
        w = np.asarray(w, dtype=np.float64)
        w0, w1, w2 = (V(w[:, k]) for k in range(3))
        Rcm = [V(cams[:, k]) for k in range(9)]
        t = [V(cams[:, 9 + k]) for k in range(3)]
        f, k1, k2 = (V(cams[:, 12 + k]) for k in range(3))
    R = [Rcm[3 * (i % 3) + i // 3] for i in range(9)]                  # fill_camblk: row-major
    Jl = left_jacobian(w0, w1, w2, mutations)
    Xv = [V(X[:, k]) for k in range(3)]
    # project_head
    qx = dot3(R[0:3], Xv) + t[0]
    qy = dot3(R[3:6], Xv) + t[1]
    qz = dot3(R[6:9], Xv) + t[2]
    px, py = (-qx) / qz, (-qy) / qz                                    # div2_shared: IEEE quotients
    n = px * px + py * py
    # project_obs: |p|^4 = pow(sqrt(n), 4) when k2 != 0, n * n otherwise (exact alike when k2 == 0)
    nz = k2.v != 0.0
    n4 = where(nz, vpow4(vsqrt(n)), n * n)
    rad = (1.0 + k1 * n) + k2 * n4
    # jacobian_obs
    iz = vrcp(qz)
    s = (-f) * iz
    c = fma(k2.exact_scale(4.0), n, k1.exact_scale(2.0))
    cpx = c * px
    B00, B01, B11 = fma(cpx, px, rad), cpx * py, fma(c * py, py, rad)
    g = fma(c, n, rad)
    a00, a01, a02 = s * B00, s * B01, s * px * g
    a10, a11, a12 = s * B01, s * B11, s * py * g
    yx, yy, yz = qx - t[0], qy - t[1], qz - t[2]
    v0 = (fma(yy, a02, -(yz * a01)), fma(yz, a00, -(yx * a02)), fma(yx, a01, -(yy * a00)))
    v1 = (fma(yy, a12, -(yz * a11)), fma(yz, a10, -(yx * a12)), fma(yx, a11, -(yy * a10)))
    jc = [[None] * 9 for _ in range(2)]
    jp = [[None] * 3 for _ in range(2)]
    for j in range(3):
        jc[0][j] = fma(v0[2], Jl[6 + j], fma(v0[1], Jl[3 + j], v0[0] * Jl[j]))
        jc[1][j] = fma(v1[2], Jl[6 + j], fma(v1[1], Jl[3 + j], v1[0] * Jl[j]))
        jp[0][j] = fma(a02, R[6 + j], fma(a01, R[3 + j], a00 * R[j]))
        jp[1][j] = fma(a12, R[6 + j], fma(a11, R[3 + j], a10 * R[j]))
    jc[0][3:6] = [a00, a01, a02]
    jc[1][3:6] = [a10, a11, a12]
    fn = f * n
    fnn = fn * n
    jc[0][6:9] = [rad * px, fn * px, fnn * px]
    jc[1][6:9] = [rad * py, fn * py, fnn * py]
    return jc, jp, dict(R=R, Jl=Jl, px=px, py=py, n=n, rad=rad, qz=qz)


def stack(jc, jp):
    """lists of V -> (values Jc [n,2,9], E [n,2,9], values Jp [n,2,3], E [n,2,3])"""
    Jc = np.stack([np.stack([x.v for x in row], axis=-1) for row in jc], axis=1)
    Ec = np.stack([np.stack([x.e for x in row], axis=-1) for row in jc], axis=1)
    Jp = np.stack([np.stack([x.v for x in row], axis=-1) for row in jp], axis=1)
    Ep = np.stack([np.stack([x.e for x in row], axis=-1) for row in jp], axis=1)
    return Jc, Ec, Jp, Ep


def bounds(mode, cams, X, w=None, mutations=()):
    """(Jc, Ec, Jp, Ep) of the restated kernel; with `mutations` the values are the mutated kernel's and the bounds the
    kernel's as it is (a mutation must not move the yardstick)"""
    Jc, Ec, Jp, Ep = stack(*kernel_f64(mode, cams, X, w)[:2])
    if mutations:
        Jc, _, Jp, _ = stack(*kernel_f64(mode, cams, X, w, mutations)[:2])
    return Jc, Ec, Jp, Ep


def tolerance(E, ref):
    return C * E + np.abs(ref).astype(np.float64) * 2.0 ** -60 + FLOOR


def excess(dev, ref, E):
    """|dev - ref| / tolerance, elementwise (<= 1 passes); dev f64, ref longdouble"""
    err = np.abs(np.asarray(dev, dtype=LD) - ref).astype(np.float64)
    return err / tolerance(E, ref)


def worst_report(dev, ref, E, names, label):
    """'' if every entry is inside its bound, else a message naming the family, the column and the worst |err| / E"""
    x = excess(dev, ref, E)
    if np.all(x <= 1.0):
        return ""
    err = np.abs(np.asarray(dev, dtype=LD) - ref).astype(np.float64)
    lines = ["%s: %d of %d entries outside C E (C = %g)" % (label, int(np.sum(x > 1.0)), x.size, C)]
    flat = x.reshape(len(x), -1)
    ncol = flat.shape[1]
    for k in range(ncol):
        col = flat[:, k]
        if np.any(col > 1.0):
            i = int(np.argmax(col))
            e = E.reshape(len(E), -1)[i, k]
            lines.append("  row %s col %s: %d bad; worst obs %d |err| = %.3e, E = %.3e, |err|/E = %.3g"
                         % ("uv"[k // len(names)], names[k % len(names)], int(np.sum(col > 1.0)), i,
                            err.reshape(len(err), -1)[i, k], e, err.reshape(len(err), -1)[i, k] / max(e, 1e-300)))
    return "\n".join(lines)


def ratio(dev, ref, E):
    """worst |err| / E (how much of the bound is used: the tolerance is C times it)"""
    err = np.abs(np.asarray(dev, dtype=LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.maximum(E, FLOOR))
    return float(np.max(r)) if r.size else 0.0


# ==================================================================================================================
# the families of cameras and points the tests draw
# ==================================================================================================================
FAMILIES = ("angles", "pixel", "geometry")
ANGLES = (0.0, 1e-12, 1.4e-8, 1.6e-8, 1e-4, 0.1 * (1 - 2.0 ** -40), 0.1 * (1 + 2.0 ** -40), 0.2, 0.3, 1.0,
          np.pi - 1e-6, np.pi + 1e-6)


def _unit(rng, m):
    d = rng.normal(size=(m, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def to_world(bal9, q):
    """X with exp(w) X + t = q (rounded to f64 from longdouble)"""
    R = exp_so3(np.asarray(bal9, dtype=np.float64)[:, 0:3])
    d = np.asarray(q, dtype=LD) - np.asarray(bal9, dtype=LD)[:, 3:6]
    return np.einsum("nji,nj->ni", R, d).astype(np.float64)


def family(name, m, seed, mode="bal", per_cam=1):
    """m observations of family `name` on m // per_cam cameras (observation i sees camera i // per_cam, one point each):
    returns (bal9 [n_cam, 9], cam_of [m], X [m, 3], label [m]).
      angles    |w| at each branch point of from_rodrigues (theta2 = f64::EPSILON at |w| = 1.49e-8) and left_jacobian
                (t2 = 1e-2 at |w| = 0.1), pi +- 1e-6, and (pi, 2 pi) in bal mode; half the cameras at pixel scale;
      pixel     f in [300, 3000], BAL-like k1 and k2, k2 zero on about half the cameras (the mixed-k2 patterns) and +-0 /
                +-5e-324 on some;
      geometry  points on the optical axis (R = I, p = 0 exactly), |p| up to 3, far points (z ~ -1e5), near-plane points
                (z up to -1e-6), cameras 1e4 from the origin with points near the camera and near the origin."""
    rng = np.random.default_rng(seed)
    nc = -(-m // per_cam)
    cam_of = np.arange(m) // per_cam
    w = rng.uniform(-np.pi, np.pi, size=(nc, 3)) * rng.uniform(0.0, 1.0, size=(nc, 1))
    t = rng.uniform(-5, 5, size=(nc, 3))
    f = rng.uniform(0.8, 1.2, nc)
    k1, k2 = rng.uniform(-1e-2, 1e-2, nc), rng.uniform(-1e-2, 1e-2, nc)
    z = -rng.uniform(1.0, 10.0, m)
    pxy = rng.uniform(-1.2, 1.2, size=(m, 2))
    lab = np.full(m, name, dtype=object)
    pix = rng.random(nc) < 0.5
    if name == "angles":
        mags = list(ANGLES) + ([np.pi + 0.5, 4.0, 5.5, 2 * np.pi - 1e-3] if mode == "bal" else [])
        mag = np.array(mags)[np.arange(nc) % len(mags)]
        w = _unit(rng, nc) * mag[:, None]
        lab = np.array(["|w|=%.3g" % x for x in mag], dtype=object)[cam_of]
        f = np.where(pix, rng.uniform(300, 3000, nc), f)
        k1 = np.where(pix, rng.uniform(-0.5, 0.5, nc), k1)
        k2 = np.where(pix, rng.uniform(-0.5, 0.5, nc), k2)
    elif name == "pixel":
        f = rng.uniform(300, 3000, nc)
        k1 = rng.uniform(-0.5, 0.5, nc) * 10.0 ** rng.uniform(-3, 0, nc)
        k2 = np.where(rng.random(nc) < 0.5, rng.uniform(-0.5, 0.5, nc) * 10.0 ** rng.uniform(-3, 0, nc), 0.0)
        k2[::16] = np.array([0.0, -0.0, 5e-324, -5e-324])[rng.integers(0, 4, len(k2[::16]))]
        pxy = rng.uniform(-1.0, 1.0, size=(m, 2))
    elif name == "geometry":
        kind_c = np.arange(nc) % 6
        kind = kind_c[cam_of]
        names = np.array(["axis", "wide", "far", "near_plane", "cam_far_pt_near_cam", "cam_far_pt_near_origin"])
        lab = names[kind].astype(object)
        pxy = np.where((kind == 1)[:, None], rng.uniform(-3, 3, size=(m, 2)) / np.sqrt(2), pxy)
        z = np.where(kind == 2, -rng.uniform(1e4, 1e5, m), z)
        z = np.where(kind == 3, -10.0 ** rng.uniform(-6, -2, m), z)
        far = (kind_c == 4) | (kind_c == 5)
        tf = _unit(rng, nc) * 1e4 * rng.uniform(1.0, 1.5, (nc, 1))
        tf[:, 2] = -np.abs(tf[:, 2]) - 5e3                              # so that the origin is in front of the camera
        t = np.where(far[:, None], tf, t)
        w[kind_c == 0] = 0.0
        f = np.where(pix, rng.uniform(300, 3000, nc), f)
        k1 = np.where(pix, rng.uniform(-0.3, 0.3, nc), k1)
        k2 = np.where(pix & (rng.random(nc) < 0.5), rng.uniform(-0.3, 0.3, nc), np.where(pix, 0.0, k2))
    else:
        raise AssertionError(name)
    bal9 = np.ascontiguousarray(np.column_stack([w, t, f, k1, k2]))
    q = np.column_stack([pxy[:, 0] * -z, pxy[:, 1] * -z, z])
    X = to_world(bal9[cam_of], q)
    if name == "geometry":
        ax = kind == 0                               # on the optical axis: R = I exactly (w = 0), X = (-t0, -t1, z - t2)
        tc = t[cam_of]
        X[ax] = np.column_stack([-tc[ax, 0], -tc[ax, 1], z[ax] - tc[ax, 2]])
        near_o = kind == 5                           # a point within 1 of the origin, in front of the far camera
        X[near_o] = rng.uniform(-1, 1, size=(int(near_o.sum()), 3))
    return bal9, cam_of, X, lab
