"""Extended-precision reference for the noise passes (add_drift, add_drift_normalized, add_noise's entity half,
add_sin_noise) and the problem statistics, and a running error bound for the kernels' order of operations (test helper;
shared by tests/test_noiseref.py, tests/test_gpu_noise_reference.py and tests/test_gpu_f32.py).  Same structure and
conventions as tests/_jacref.py, whose LD, U, C, FLOOR and TRIG_ULP it takes.

Two halves:
  * reference, np.longdouble (x87 80-bit), written from the formulas of src/noise.rs and Camera::transform / center, in
    forms that do not follow the kernels': the centre is -R^T t (an orthonormal R's transpose; the kernels divide
    cofactors by a determinant), the new rotation is a plain row-major matrix product R dR, the axis-angle rotation is
    I + sin a K + (1 - cos a) K^2, distance^1.2 is long double `power`, sin / cos are long double.  The standard
    normals are INPUTS (normal_pairs: Box-Muller of the Philox4x32-10 words in long double), so the arithmetic of the
    passes is judged apart from the draw.
  * kernel half, numpy in the state's scalar type: cm_center, cm_mat_vec, cm_mat_mul, cm_from_axis_angle,
    transform_cam15 and the bodies of k_add_drift, k_add_noise_entities and k_add_sin_noise restated in the device's
    order (no contraction: the kernels are compiled with -ffp-contract=off), carrying beside every value a first-order
    running bound E: each rounded operation adds u |result|, every (T) conversion one more rounding, sin / cos their
    ulp bound plus the propagated error of the angle, pow its bound (below).  u = 2^-53 gives the bound of the double
    kernels, u = 2^-24 that of the float instantiations.

What enters E besides roundings:
  * the draws: the device evaluates Box-Muller through log_unit / sincos_turns (fdlibm kernels, < 1 ulp each): the
    radius sqrt(-2 ln u1) is within 2 u, the turn-reduced sine / cosine keep RELATIVE accuracy (one rounding of the
    reduced argument, 1 ulp of the kernel) and the product adds one: 6 u |z|.  The CPU oracle takes libm's cos of
    the rounded angle 2 pi u2 instead: 4 pi u absolute on the cosine, i.e. 13 u times the radius.  The kernels' bound
    carries DRAW_REL |z| alone; DRAW_ABS radius is added only where the oracle is the one being judged (oracle=True:
    tests/test_noiseref.py), so that it does not widen what the kernels are held to.
  * pow_lean(d, 1.2) = exp_lean(1.2 log_unit(d)): the logarithm's ulp (2 u relative) and the product's rounding are
    amplified by |l| = |1.2 ln d| in the exponential, which adds its own ulp: (3 |l| + 3) u relative.  powf (float):
    ocml's documented 16 ulp, and 1.2f is not 1.2: |ln d| u more.
  * sin / cos: TRIG_ULP (double), 4 ulp for the float functions (the OpenCL full-profile bounds ocml documents); capped
    at 2, the distance of any two sines.  Where the cap binds the case is UNRESOLVED in that scalar type (resolved()):
    the float sine pass on the planar cloud has angles of ~1e8 rad known to tens of radians.
  * the reference's own centre: -R^T t equals -R^-1 t up to (R^T R - I) c; |R^T R - I| |c| is added to the centre's
    bound (R is a rotation rounded to the scalar type, so this is a few u |c|).

Statistics (stats_bound; D = the number of roundings along the longest accumulation path, M = max |x|, R = max - min):
  * mean: sum of x_i / n in ANY order of depth D: |err| <= (D + 2) u mean|x_i|  (one rounding per level, the reciprocal and
    the product; a sequential fold has D = n, the device's tree D = device_depth(n));
  * every partial mean is therefore within e_mu = (D + 2) u M;
  * M2 = sum (x - mean)^2, two-pass within a batch and merged by Chan's update delta^2 n_a n_b / n: the deviations are
    exact differences of nearby numbers (u |dx| each), so the sums of squares carry (D + 4) u M2; a batch taken around
    an inexact mean gains n e_mu^2 (exactly: sum (x - m')^2 = sum (x - m)^2 + n (m - m')^2); every merge sees delta off
    by 2 e_mu: 2 |delta| 2 e_mu w with |delta| <= R and the weights w = n_a n_b / n summing to at most n per level:
        E_M2 = (D + 4) u M2 + 4 R e_mu n D + n e_mu^2
    -- the u (1 + |mean| / sigma) terms: relative to M2 = n sigma^2 the middle one is ~ D^2 u (M / sigma);
  * std = sqrt(M2 / n): E_M2 / (2 n sigma) + 2 u sigma (sqrt(E_M2 / n) when sigma = 0); |std| likewise from the three.
  min, max and the origin are selections: compared exactly; dimensions = max - min is one rounded subtraction of
  them (u |dimension| against the long-double difference; exact against the f64 difference of the rounded extremes,
  exact_slots()).

An entry passes when |dev - ref| <= C E + |ref| 2^-60 + FLOOR (tolerance(), _jacref's C and FLOOR).  `mutations`
switches one-line changes of the restated kernels on (tests/test_noiseref.py shows each lands outside the bound)."""
import numpy as np

from _jacref import LD, U, C, FLOOR, TRIG_ULP, tolerance, excess, ratio  # noqa: F401  (re-exported)

U32 = 2.0 ** -24            # unit roundoff of f32
F32_TRIG_ULP = 4.0          # sinf / cosf / sincosf: OpenCL full profile (what ocml documents)
F32_POW_ULP = 16.0          # powf: the same table
TRIG_CAP = 2.0              # two values in [-1, 1] are never further apart: an angle known to worse than a radian says nothing
DRAW_REL = 6.0              # device draw: 6 u |z|            (module docstring)
DRAW_ABS = 13.0             # libm cos(2 pi u2) of the oracle: 13 u radius (oracle=True only)
STREAM_DRIFT_CAM, STREAM_DRIFT_PT, STREAM_NOISE_CAM, STREAM_NOISE_PT = 1, 2, 3, 4       # camera_math.hpp
STAT_BLOCK, STAT_GRID, STAT_BATCH = 256, 512, 4                                        # kernels.hpp: k_stats_pass1's shape

MUTATIONS = ("dR_R", "center_R", "rot_y", "pow_1", "dist_1", "draws_swapped", "no_bal_std", "no_eps", "noise_dir_raw",
             "chan_nb", "origin_tie_earlier")
MUTATION_TEXT = {
    "dR_R": "dR R in place of R dR",
    "center_R": "the centre taken with R in place of its inverse",
    "rot_y": "the drift's rotation about y in place of x",
    "pow_1": "d**1.0 in place of d**1.2",
    "dist_1": "distance in place of distance^2",
    "draws_swapped": "the angle draw and the translation draw swapped",
    "no_bal_std": "bal_std dropped from the camera translation",
    "no_eps": "the 1e-8 substitution missing",
    "noise_dir_raw": "noise_dir not normalised",
    "chan_nb": "n_a n_b / n replaced by n_b in the Chan merge",
    "origin_tie_earlier": "the origin's tie going to the earlier entity",
}


# ==================================================================================================================
# the draws: Philox4x32-10 (vectorised) and Box-Muller in long double
# ==================================================================================================================
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """the four output words for arrays of counters (uint64 arithmetic on 32-bit values)"""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & m32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def uniforms(seed, stream, entities, slot):
    """(u1 in (0, 1], u2 in [0, 1)) of normal_pair(seed; stream, entity, slot), exact in long double"""
    ent = np.asarray(entities, dtype=np.uint64)
    o = philox4x32_10(ent, ent >> np.uint64(32), slot, stream, int(seed), int(seed) >> 32)
    a = (o[1] << np.uint64(32)) | o[0]
    b = (o[3] << np.uint64(32)) | o[2]
    u1 = ((a >> np.uint64(11)).astype(LD) + 1) * LD(2.0 ** -53)
    u2 = (b >> np.uint64(11)).astype(LD) * LD(2.0 ** -53)
    return u1, u2


_PI_LD = LD(4) * np.arctan(LD(1))


def normal_pairs(seed, stream, entities, slots):
    """[n, len(slots), 2] standard normals in long double: (z0, z1) = sqrt(-2 ln u1) (cos, sin)(2 pi u2); the angle is
    reduced in exact arithmetic first (8 u2 is exact), so that the result is as good as long double gets"""
    ent = np.asarray(entities, dtype=np.uint64)
    out = np.empty((len(ent), len(slots), 2), dtype=LD)
    for k, slot in enumerate(slots):
        u1, u2 = uniforms(seed, stream, ent, slot)
        rad = np.sqrt(-2 * np.log(u1))
        t = 4 * u2
        q = np.rint(t)
        x = (t - q) * (_PI_LD / 2)                           # in [-pi/4, pi/4]
        s, c = np.sin(x), np.cos(x)
        qi = q.astype(np.int64) & 3
        cs = np.select([qi == 0, qi == 1, qi == 2], [c, -s, -c], s)
        sn = np.select([qi == 0, qi == 1, qi == 2], [s, c, -s], -c)
        out[:, k, 0] = rad * cs
        out[:, k, 1] = rad * sn
    return out


def drift_draws(seed, n_cam, n_pts, cam_base=0):
    """(z_cam [n_cam, 2], z_pt [n_pts, 2]) of k_add_drift: slot 0 of the two drift streams"""
    return (normal_pairs(seed, STREAM_DRIFT_CAM, np.arange(n_cam) + cam_base, (0,))[:, 0],
            normal_pairs(seed, STREAM_DRIFT_PT, np.arange(n_pts), (0,))[:, 0])


def noise_draws(seed, n_cam, n_pts, cam_base=0):
    """(draws_cam [n_cam, 4, 2], draws_pt [n_pts, 2, 2]) of k_add_noise_entities"""
    return (normal_pairs(seed, STREAM_NOISE_CAM, np.arange(n_cam) + cam_base, (0, 1, 2, 3)),
            normal_pairs(seed, STREAM_NOISE_PT, np.arange(n_pts), (0, 1)))


# ==================================================================================================================
# reference (longdouble)
# ==================================================================================================================
def _ld(a, shape):
    return np.asarray(a, dtype=LD).reshape(shape)


def _rot(c):
    """row-major R [n, r, c] of cam15 rows (columns 0..8 are column-major)"""
    return c[:, 0:9].reshape(-1, 3, 3).transpose(0, 2, 1)


def centers(cams15):
    """-R^T t [n, 3] (longdouble)"""
    c = _ld(cams15, (-1, 15))
    return -np.einsum("nji,nj->ni", _rot(c), c[:, 9:12])


def transform(cams15, dR, dloc):
    """Camera::transform: dir = dir * delta_dir, loc = -(dir (center + delta_loc)) with the OLD dir; dR row-major
    [n, 3, 3]; returns cam15 rows (longdouble)"""
    c = _ld(cams15, (-1, 15))
    R = _rot(c)
    out = c.copy()
    out[:, 0:9] = (R @ dR).transpose(0, 2, 1).reshape(-1, 9)
    out[:, 9:12] = -np.einsum("nij,nj->ni", R, centers(c) + dloc)
    return out


def _rot_x(a):
    s, c = np.sin(a), np.cos(a)
    M = np.zeros(a.shape + (3, 3), dtype=LD)
    M[:, 0, 0] = 1
    M[:, 1, 1], M[:, 1, 2], M[:, 2, 1], M[:, 2, 2] = c, -s, s, c
    return M


def _axis_angle(ax, a):
    K = np.zeros(a.shape + (3, 3), dtype=LD)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -ax[:, 2], ax[:, 1], -ax[:, 0]
    K[:, 1, 0], K[:, 2, 0], K[:, 2, 1] = ax[:, 2], -ax[:, 1], ax[:, 0]
    return np.eye(3, dtype=LD) + np.sin(a)[:, None, None] * K + (1 - np.cos(a))[:, None, None] * (K @ K)


def _norm(v):
    return np.sqrt((v * v).sum(axis=-1))


def drift(cams15, pts, origin, strength, angle_strength, std, dir, z_cam, z_pt):      # noqa: A002
    """add_drift (src/noise.rs:68-116): returns (cams15, pts, info) in longdouble; info = dict(d_cam, d_pt, angle)"""
    c, p = _ld(cams15, (-1, 15)), _ld(pts, (-1, 3))
    o, d3 = _ld(origin, 3), _ld(dir, 3)
    zc, zp = _ld(z_cam, (-1, 2)), _ld(z_pt, (-1, 2))
    strength, angle_strength, std = LD(strength), LD(angle_strength), LD(std)
    dc = _norm(centers(c) - o)
    angle = angle_strength * (1 + std * zc[:, 0]) * np.power(dc, LD(np.float64(1.2)))
    move = d3[None, :] * (strength * (1 + std * zc[:, 1]) * dc * dc)[:, None]
    cams = transform(c, _rot_x(angle), move)
    dp = _norm(p - o)
    out_p = p + d3[None, :] * (strength * (1 + std * zp[:, 0]) * dp * dp)[:, None]
    return cams, out_p, dict(d_cam=dc, d_pt=dp, angle=angle, move=move)


def drift_normalized(cams15, pts, origin, strength, angle_strength, std, z_cam, z_pt, std3):
    """add_drift_normalized (src/noise.rs:47-56): dir = std().normalize(), strength * |std()|"""
    s = _ld(std3, 3)
    mag = _norm(s)
    return drift(cams15, pts, origin, LD(strength) * mag, angle_strength, std, s / mag, z_cam, z_pt)


def noise_entities(cams15, pts, bal_std, translation_std, rotation_std, point_std, draws_cam, draws_pt):
    """add_noise's cameras and points (src/noise.rs:129-150).  draws_cam [n, 4, 2]: slots 0..3 of the camera stream
    -> axis (z00, z01, z10), rotation z11, direction (z20, z21, z30), translation z31; draws_pt [n, 2, 2]: direction
    (z00, z01, z10), magnitude z11."""
    c, p = _ld(cams15, (-1, 15)), _ld(pts, (-1, 3))
    zc, zp = _ld(draws_cam, (-1, 4, 2)), _ld(draws_pt, (-1, 2, 2))
    a = np.stack([zc[:, 0, 0], zc[:, 0, 1], zc[:, 1, 0]], axis=1)
    b = np.stack([zc[:, 2, 0], zc[:, 2, 1], zc[:, 3, 0]], axis=1)
    a = a / _norm(a)[:, None]
    b = b / _norm(b)[:, None]
    cams = transform(c, _axis_angle(a, LD(rotation_std) * zc[:, 1, 1]), b * (LD(bal_std) * LD(translation_std) * zc[:, 3, 1])[:, None])
    q = np.stack([zp[:, 0, 0], zp[:, 0, 1], zp[:, 1, 0]], axis=1)
    q = q / _norm(q)[:, None]
    return cams, p + q * (LD(point_std) * zp[:, 1, 1])[:, None]


def sin_noise(cams15, pts, dimensions, dir, noise_dir, strength, frequency):          # noqa: A002
    """add_sin_noise (src/noise.rs:388-416); the reference multiplies by the f64 constant PI"""
    c, p = _ld(cams15, (-1, 15)), _ld(pts, (-1, 3))
    dim = _ld(dimensions, 3).copy()
    dim[dim == 0] = LD(np.float64(1e-8))
    d3, n3 = _ld(dir, 3), _ld(noise_dir, 3)
    n3 = n3 / _norm(n3)

    def wave(x):
        return np.sin(((x / dim) * d3).sum(axis=1) * LD(frequency) * LD(np.float64(np.pi))) * LD(strength)
    cams = transform(c, np.broadcast_to(np.eye(3, dtype=LD), (len(c), 3, 3)), n3[None, :] * wave(centers(c))[:, None])
    return cams, p + n3[None, :] * wave(p)[:, None]


def origin_index(ent):
    """fold1's rule (src/noise.rs:80-86) on the ROUNDED distances: strict <, so among equal distances the later entity.
    Raises if two different distances are closer than the reference's own f64 evaluation could tell apart (8 ulps): such
    an input has no defined answer here."""
    e = np.asarray(ent, dtype=LD)
    d = np.sqrt((e * e).sum(axis=1)).astype(np.float64)
    lo = d.min()
    near = d[(d > lo) & (d <= lo * (1 + 16 * U))]
    if near.size:
        raise ValueError("origin: %d distances within 8 ulps of the smallest without being equal to it" % near.size)
    return int(np.flatnonzero(d == lo)[-1])


def statistics(cams15, pts, centers_=None):
    """the 20-slot record in longdouble: mean 0..2, std 3..5, min 6..8, max 9..11, dimensions 12..14, origin 15..17,
    origin index 18, |std| 19 -- two-pass around the finished mean.  centers_ (f64 [n_cam, 3]): take these as the
    cameras' centres (the device's statistics read the centres a kernel computed) instead of -R^T t."""
    cen = centers(cams15) if centers_ is None else _ld(centers_, (-1, 3))
    ent = np.concatenate([cen, _ld(pts, (-1, 3))], axis=0)
    n = len(ent)
    rec = np.zeros(20, dtype=LD)
    mean = ent.sum(axis=0) / n
    sd = np.sqrt(((ent - mean) ** 2).sum(axis=0) / n)
    rec[0:3], rec[3:6] = mean, sd
    rec[6:9], rec[9:12] = ent.min(axis=0), ent.max(axis=0)
    rec[12:15] = rec[9:12] - rec[6:9]
    i = origin_index(ent)
    rec[15:18], rec[18] = ent[i], i
    rec[19] = _norm(sd)
    return rec


# ==================================================================================================================
# the kernels' order in the state's scalar type, with a running error bound
# ==================================================================================================================
def _abs64(x):
    return np.abs(np.asarray(x, dtype=np.float64))


class Arith:
    """the scalar type T of a kernel instantiation: u = 2^-53 -> double, u = 2^-24 -> float"""

    def __init__(self, u=U):
        assert u in (U, U32)
        self.u = float(u)
        self.dt = np.float64 if u == U else np.float32
        self.trig_ulp = TRIG_ULP if u == U else F32_TRIG_ULP

    def val(self, v, e=None):
        """a value of type T that is an INPUT (exact unless e is given)"""
        return X(self, np.asarray(v, dtype=self.dt), e)

    def cast(self, v64, e=None):
        """(T) of a double (value v64 with bound e): one rounding when T is float"""
        v = np.asarray(np.asarray(v64, dtype=np.float64), dtype=self.dt)
        e = np.zeros(v.shape) if e is None else np.asarray(e, dtype=np.float64)
        return X(self, v, e + (self.u * _abs64(v) if self.dt is np.float32 else 0.0))


class X:
    """value (type T, the kernel's rounding) and E >= |value - exact| (f64), elementwise"""
    __slots__ = ("a", "v", "e")

    def __init__(self, a, v, e=None):
        self.a = a
        self.v = np.asarray(v, dtype=a.dt)
        self.e = np.zeros(self.v.shape) if e is None else np.asarray(e, dtype=np.float64)

    def _w(self, o):
        return o if isinstance(o, X) else X(self.a, self.a.dt(o))          # 0, 1, -1: exact in either type

    def _r(self, v, prop):
        return X(self.a, v, prop + self.a.u * _abs64(v))

    def __add__(self, o):
        o = self._w(o)
        return self._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = self._w(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return self._w(o) - self

    def __mul__(self, o):
        o = self._w(o)
        return self._r(self.v * o.v, _abs64(o.v) * self.e + _abs64(self.v) * o.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._w(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.v / o.v
            d = _abs64(o.v)
            rel = np.minimum(o.e / d, 0.5)
            return self._r(v, (self.e + _abs64(v) * o.e) / (d * (1 - rel)))

    def __rtruediv__(self, o):
        return self._w(o) / self

    def __neg__(self):
        return X(self.a, -self.v, self.e)

    def __getitem__(self, k):
        return X(self.a, self.v[k], self.e[k])


def xsqrt(x):
    v = np.sqrt(x.v)
    v64 = _abs64(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        prop = np.where(v64 > 0, x.e / (2 * np.where(v64 > 0, v64, 1.0)), np.sqrt(x.e))
    return x._r(v, prop)


def _trig(x, fn, dfn):
    """sin / cos of the rounded angle: the library's ulp bound (one ulp <= 2 u |result|) plus the angle's own error"""
    v = fn(x.v.astype(LD)).astype(x.a.dt)
    e = _abs64(dfn(x.v.astype(np.float64))) * x.e + 0.5 * x.e * x.e + 2 * x.a.trig_ulp * x.a.u * _abs64(v)
    return X(x.a, v, np.minimum(e, TRIG_CAP))


def xsin(x):
    return _trig(x, np.sin, np.cos)


def xcos(x):
    return _trig(x, np.cos, np.sin)


def xpow12(d, expo=1.2):
    """pow_t(distance, (T)1.2): pow_lean for double, powf for float (module docstring); d >= 0"""
    a = d.a
    y = np.float64(a.dt(expo))
    v = np.power(d.v.astype(LD), LD(y)).astype(a.dt)
    v64, d64 = _abs64(v), _abs64(d.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        lnd = np.where(d64 > 0, np.abs(np.log(np.where(d64 > 0, d64, 1.0))), 0.0)
    own = (3 * y * lnd + 3) * a.u * v64 if a.dt is np.float64 else (2 * F32_POW_ULP + 1.2 * lnd) * a.u * v64
    prop = y * (d64 + d.e) ** (y - 1) * d.e                            # the derivative grows with d: its value at the far end
    return X(a, v, prop + own)


def xdot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cm_center(m, t, mutations=()):
    """-(R^-1 t) by cofactors over the determinant; m = the 9 column-major entries"""
    if "center_R" in mutations:
        return [-x for x in cm_mat_vec(m, t)]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m
    det = m00 * (m11 * m22 - m21 * m12) - m10 * (m01 * m22 - m21 * m02) + m20 * (m01 * m12 - m11 * m02)
    a = ((m11 * m22 - m12 * m21) / det, (m12 * m20 - m10 * m22) / det, (m10 * m21 - m11 * m20) / det)
    b = ((m21 * m02 - m22 * m01) / det, (m22 * m00 - m20 * m02) / det, (m20 * m01 - m21 * m00) / det)
    c = ((m01 * m12 - m02 * m11) / det, (m02 * m10 - m00 * m12) / det, (m00 * m11 - m01 * m10) / det)
    return [-xdot3(a, t), -xdot3(b, t), -xdot3(c, t)]


def cm_mat_vec(m, x):
    return [xdot3((m[0], m[3], m[6]), x), xdot3((m[1], m[4], m[7]), x), xdot3((m[2], m[5], m[8]), x)]


def cm_mat_mul(a, b):
    return [xdot3((a[r], a[3 + r], a[6 + r]), (b[3 * c], b[3 * c + 1], b[3 * c + 2])) for c in range(3) for r in range(3)]


def cm_from_axis_angle(ax, ay, az, angle):
    s, c = xsin(angle), xcos(angle)
    k = 1.0 - c
    return [k * ax * ax + c, k * ax * ay + s * az, k * ax * az - s * ay,
            k * ax * ay - s * az, k * ay * ay + c, k * ay * az + s * ax,
            k * ax * az + s * ay, k * ay * az - s * ax, k * az * az + c]


class Cams:
    """cam15 columns as X, the centre the kernels compute (with the reference's own slack, module docstring)"""

    def __init__(self, a, cams15, mutations=()):
        c = np.asarray(cams15, dtype=a.dt).reshape(-1, 15)
        self.a, self.raw, self.n = a, c, len(c)
        self.m = [a.val(c[:, k]) for k in range(9)]
        self.t = [a.val(c[:, 9 + k]) for k in range(3)]
        ctr = cm_center(self.m, self.t, mutations)
        cl = c.astype(LD)
        R = _rot(cl)
        defect = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3, dtype=LD)).astype(np.float64)      # |R^T R - I|
        slack = np.einsum("nij,nj->ni", defect, np.abs(centers(cl)).astype(np.float64))
        self.ctr = [X(a, ctr[k].v, ctr[k].e + slack[:, k]) for k in range(3)]

    def transform(self, dR, d, mutations=()):
        """transform_cam15 -> [n, 15] values and bounds (columns 12..14: the input's bits, bound 0)"""
        v = cm_mat_vec(self.m, [self.ctr[k] + d[k] for k in range(3)])
        nr = cm_mat_mul(dR, self.m) if "dR_R" in mutations else cm_mat_mul(self.m, dR)
        cols = nr + [-1.0 * x for x in v]
        val = np.concatenate([np.stack([np.broadcast_to(x.v, (self.n,)) for x in cols], axis=1), self.raw[:, 12:15]], axis=1)
        err = np.concatenate([np.stack([np.broadcast_to(x.e, (self.n,)) for x in cols], axis=1), np.zeros((self.n, 3))], axis=1)
        return val, err


def _draw(z, oracle=False):
    """the draw itself: z [n, 2] longdouble pairs -> (value f64 [n, 2], bound [n, 2]) of what the device's normal_pair
    returns (oracle: what the CPU oracle's libm evaluation returns)"""
    z = np.asarray(z, dtype=LD).reshape(-1, 2)
    v = z.astype(np.float64)
    rad = np.sqrt((v * v).sum(axis=1, keepdims=True))
    return v, U * (DRAW_REL * np.abs(v) + (DRAW_ABS * rad if oracle else 0.0)) + np.abs(z - v).astype(np.float64)


def _draw_lin(a, base, std, zv, ze):
    """(T)(base + std * z), the double arithmetic of the kernels' draw lines"""
    prod = np.float64(std) * zv
    v = base + prod
    return a.cast(v, abs(float(std)) * ze + U * np.abs(prod) + U * np.abs(v))


def _points(a, pts):
    p = np.asarray(pts, dtype=a.dt).reshape(-1, 3)
    return [a.val(p[:, k]) for k in range(3)]


def _stack(cols):
    n = max([np.ndim(x.v) and len(x.v) for x in cols] + [0])
    return (np.stack([np.broadcast_to(x.v, (n,)) for x in cols], axis=1), np.stack([np.broadcast_to(x.e, (n,)) for x in cols], axis=1))


def k_add_drift(cams15, pts, origin, strength, angle_strength, std, dir, z_cam, z_pt, u=U, std3=None, mutations=(),    # noqa: A002
                oracle=False):
    """k_add_drift<T> restated: returns (cams [n, 15], E_cams, pts [n, 3], E_pts).  std3 = stats[3..5]: the
    add_drift_normalized entry (dir and strength derived in double, as the kernel does)."""
    a = Arith(u)
    d64 = Arith(U)
    if std3 is not None:
        s = [d64.val(np.float64(x)) for x in std3]
        mag = xsqrt(xdot3(s, s))
        inv = 1.0 / mag
        dirx = [s[k] * inv for k in range(3)]
        st = d64.val(np.float64(strength)) * mag
    else:
        dirx = [d64.val(np.float64(x)) for x in dir]
        st = d64.val(np.float64(strength))
    dx, dy, dz = (a.cast(x.v, x.e) for x in dirx)
    st = a.cast(st.v, st.e)
    ast = a.cast(np.float64(angle_strength))
    o = [a.cast(np.float64(x)) for x in origin]
    zc, ezc = _draw(z_cam, oracle)
    zp, ezp = _draw(z_pt, oracle)
    ia, it = (1, 0) if "draws_swapped" in mutations else (0, 1)

    def dist(x):
        e = [x[k] - o[k] for k in range(3)]
        return xsqrt(xdot3(e, e))

    def move(dk, v, distance):
        m = dk * st * v * distance
        return m if "dist_1" in mutations else m * distance
    cm = Cams(a, cams15, mutations)
    distance = dist(cm.ctr)
    va = _draw_lin(a, 1.0, std, zc[:, ia], ezc[:, ia])
    vt = _draw_lin(a, 1.0, std, zc[:, it], ezc[:, it])
    angle = ast * va * (distance if "pow_1" in mutations else xpow12(distance))
    sn, cs = xsin(angle), xcos(angle)
    one, zero = a.val(np.ones(cm.n)), a.val(np.zeros(cm.n))
    if "rot_y" in mutations:
        dR = [cs, zero, -sn, zero, one, zero, sn, zero, cs]
    else:
        dR = [one, zero, zero, zero, cs, sn, zero, -sn, cs]
    cv, ce = cm.transform(dR, [move(dx, vt, distance), move(dy, vt, distance), move(dz, vt, distance)], mutations)
    p = _points(a, pts)
    dp = dist(p)
    v = _draw_lin(a, 1.0, std, zp[:, 0], ezp[:, 0])
    pv, pe = _stack([p[0] + move(dx, v, dp), p[1] + move(dy, v, dp), p[2] + move(dz, v, dp)])
    return cv, ce, pv, pe


def k_add_noise_entities(cams15, pts, bal_std, translation_std, rotation_std, point_std, draws_cam, draws_pt, u=U,
                         mutations=(), oracle=False):
    a = Arith(u)
    zc = np.asarray(draws_cam, dtype=LD).reshape(-1, 4, 2)
    zp = np.asarray(draws_pt, dtype=LD).reshape(-1, 2, 2)
    dc = [_draw(zc[:, k], oracle) for k in range(4)]
    dp = [_draw(zp[:, k], oracle) for k in range(2)]

    def unit(parts):
        q = [a.cast(v, e) for v, e in parts]
        inv = 1.0 / xsqrt(xdot3(q, q))
        return [x * inv for x in q]
    bs = a.cast(np.float64(bal_std))
    A = unit([(dc[0][0][:, 0], dc[0][1][:, 0]), (dc[0][0][:, 1], dc[0][1][:, 1]), (dc[1][0][:, 0], dc[1][1][:, 0])])
    B = unit([(dc[2][0][:, 0], dc[2][1][:, 0]), (dc[2][0][:, 1], dc[2][1][:, 1]), (dc[3][0][:, 0], dc[3][1][:, 0])])
    ang = _draw_lin(a, 0.0, rotation_std, dc[1][0][:, 1], dc[1][1][:, 1])
    t = _draw_lin(a, 0.0, translation_std, dc[3][0][:, 1], dc[3][1][:, 1])
    cm = Cams(a, cams15, mutations)
    dR = cm_from_axis_angle(A[0], A[1], A[2], ang)
    loc = [(B[k] * t) if "no_bal_std" in mutations else (B[k] * bs * t) for k in range(3)]
    cv, ce = cm.transform(dR, loc, mutations)
    Q = unit([(dp[0][0][:, 0], dp[0][1][:, 0]), (dp[0][0][:, 1], dp[0][1][:, 1]), (dp[1][0][:, 0], dp[1][1][:, 0])])
    mm = _draw_lin(a, 0.0, point_std, dp[1][0][:, 1], dp[1][1][:, 1])
    p = _points(a, pts)
    pv, pe = _stack([p[k] + Q[k] * mm for k in range(3)])
    return cv, ce, pv, pe


def k_add_sin_noise(cams15, pts, dimensions, dir, noise_dir, strength, frequency, u=U, mutations=()):      # noqa: A002
    a = Arith(u)
    e = np.asarray(dimensions, dtype=np.float64).copy()
    if "no_eps" not in mutations:
        e[e == 0.0] = 1e-8
    d = [a.cast(x) for x in e]
    n = [a.cast(np.float64(x)) for x in noise_dir]
    dr = [a.cast(np.float64(x)) for x in dir]
    st, fr, pi = a.cast(np.float64(strength)), a.cast(np.float64(frequency)), a.cast(np.float64(np.pi))
    if "noise_dir_raw" not in mutations:
        inv = 1.0 / xsqrt(xdot3(n, n))
        n = [x * inv for x in n]

    def wave(x):
        return xsin(xdot3([x[0] / d[0], x[1] / d[1], x[2] / d[2]], dr) * fr * pi) * st
    cm = Cams(a, cams15, mutations)
    s = wave(cm.ctr)
    one, zero = a.val(np.ones(cm.n)), a.val(np.zeros(cm.n))
    with np.errstate(invalid="ignore", over="ignore"):
        cv, ce = cm.transform([one, zero, zero, zero, one, zero, zero, zero, one], [n[k] * s for k in range(3)], mutations)
        p = _points(a, pts)
        sp = wave(p)
        pv, pe = _stack([p[k] + n[k] * sp for k in range(3)])
    return cv, ce, pv, pe


def device_centers(cams15, u=U):
    """cm_center of every camera in the device's order: (values [n, 3] of type T, bound) -- for double these are the
    bits the kernels and the camera table hold"""
    cm = Cams(Arith(u), cams15)
    return _stack(cm.ctr) if cm.n else (np.zeros((0, 3), dtype=cm.a.dt), np.zeros((0, 3)))


# ---- statistics ----------------------------------------------------------------------------------------------------
def device_depth(n):
    """roundings along the longest accumulation path of k_stats_pass1 over n entities: a thread's entities (batches of
    STAT_BATCH folded one after the other), 6 levels of the wave tree and 2 of the workgroup's, the last workgroup's
    records per thread and its 8 levels"""
    grid = max(1, min(STAT_GRID, -(-n // STAT_BLOCK)))
    per_thread = -(-n // (grid * STAT_BLOCK))
    return per_thread + 8 + -(-grid // STAT_BLOCK) + 8


def stats_bound(ent, depth, u=U, e_ent=None):
    """E [20] for the record of the entities ent [n, 3] (f64) accumulated in an order of that depth (module docstring);
    slots 6..18 are 0 (exact), or the entities' own bound e_ent for values selected from computed centres"""
    x = np.asarray(ent, dtype=LD)
    n, D = len(x), float(depth)
    E = np.zeros(20)
    mean = x.sum(axis=0) / n
    M = np.abs(x).max(axis=0).astype(np.float64)
    Rg = (x.max(axis=0) - x.min(axis=0)).astype(np.float64)
    M2 = ((x - mean) ** 2).sum(axis=0).astype(np.float64)
    E[0:3] = (D + 2) * u * (np.abs(x).sum(axis=0) / n).astype(np.float64)
    e_mu = (D + 2) * u * M
    E_M2 = (D + 4) * u * M2 + 4 * Rg * e_mu * n * D + n * e_mu * e_mu
    sd = np.sqrt(M2 / n)
    with np.errstate(divide="ignore", invalid="ignore"):
        E[3:6] = np.where(sd > 0, E_M2 / (2 * n * np.where(sd > 0, sd, 1.0)), np.sqrt(E_M2 / n)) + 2 * u * sd
    mag = float(np.sqrt((sd * sd).sum()))
    E[19] = (float((sd * E[3:6]).sum()) / mag if mag > 0 else float(np.sqrt((E[3:6] ** 2).sum()))) + 3 * u * mag
    E[12:15] = u * Rg                                   # max - min: one rounded subtraction of two selected values
    if e_ent is not None:
        worst = np.asarray(e_ent, dtype=np.float64).reshape(-1, 3).max(axis=0) if len(e_ent) else np.zeros(3)
        E[0:3] += worst
        E[3:6] += 2 * worst
        E[19] += 2 * float(np.sqrt((worst ** 2).sum()))
        E[6:9], E[9:12], E[12:15], E[15:18] = worst, worst, 2 * worst, worst
    return E


def exact_slots(ref):
    """(slots, values): the entries of a record that are selections of input values -- min, max, origin, its index -- and
    dimensions as the f64 difference of the rounded extremes (IEEE: THE correctly rounded difference)"""
    r = np.asarray(ref, dtype=LD).astype(np.float64)
    r[12:15] = r[9:12] - r[6:9]
    k = np.arange(6, 19)
    return k, r[k]


def k_stats(ent, mutations=()):
    """The statistics pass restated in f64 at its own (simpler) shape: batches of STAT_BATCH entities, each a (count,
    mean, M2) triple taken two-pass, merged pairwise in a tree by Chan's update (vectorised level by level); the mean as
    the same tree's sum of x / n; the origin by fold1's rule.  Returns (record [20] f64, depth of this order)."""
    x = np.asarray(ent, dtype=np.float64).reshape(-1, 3)
    n = len(x)
    rec = np.zeros(20)
    inv = 1.0 / n
    nb = -(-n // STAT_BATCH)
    valid = (np.arange(nb * STAT_BATCH) < n).reshape(nb, STAT_BATCH)
    xb = np.zeros((nb * STAT_BATCH, 3))
    xb[:n] = x
    xb = xb.reshape(nb, STAT_BATCH, 3)
    s, bs = np.zeros((nb, 3)), np.zeros((nb, 3))
    for u in range(STAT_BATCH):                                       # sequential within a batch, like a thread's registers
        s = np.where(valid[:, u, None], s + xb[:, u] * inv, s)
        bs = np.where(valid[:, u, None], bs + xb[:, u], bs)
    cnt = valid.sum(axis=1).astype(np.float64)
    mu = bs * (1.0 / cnt)[:, None]
    m2 = np.zeros((nb, 3))
    for u in range(STAT_BATCH):
        d = xb[:, u] - mu
        m2 = np.where(valid[:, u, None], m2 + d * d, m2)
    depth = STAT_BATCH
    while len(cnt) > 1:
        k = len(cnt) // 2 * 2
        ca, cb, ma, mb, qa, qb = cnt[0:k:2], cnt[1:k:2], mu[0:k:2], mu[1:k:2], m2[0:k:2], m2[1:k:2]
        tot = ca + cb
        f = cb / tot
        delta = mb - ma
        w = cb if "chan_nb" in mutations else ca * f
        parts = (tot, ma + delta * f[:, None], (qa + qb) + (delta * delta) * w[:, None], s[0:k:2] + s[1:k:2])
        cnt, mu, m2, s = (np.concatenate([p, r[k:]]) for p, r in zip(parts, (cnt, mu, m2, s)))
        depth += 1
    rec[0:3] = s[0]
    sd = np.sqrt(m2[0] / n)
    rec[3:6] = sd
    rec[19] = np.sqrt((sd[0] * sd[0] + sd[1] * sd[1]) + sd[2] * sd[2])
    rec[6:9], rec[9:12] = x.min(axis=0), x.max(axis=0)
    rec[12:15] = rec[9:12] - rec[6:9]
    d = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
    hits = np.flatnonzero(d == d.min())
    i = int(hits[0] if "origin_tie_earlier" in mutations else hits[-1])
    rec[15:18], rec[18] = x[i], i
    return rec, depth + 2


def stats_record(cams15, pts):
    """The 20 doubles a correct statistics pass hands the noise kernels for this state: the reference's record rounded
    to f64, taken over the centres as the device computes them (so that an origin that is a camera carries the bits
    the kernel will subtract)."""
    cen = device_centers(cams15)[0]
    return statistics(cams15, pts, centers_=cen).astype(np.float64)


def outside(dev, ref, E):
    """elementwise: the entry misses its bound.  Where the reference itself is NaN (add_drift_normalized of a single
    entity: std() = 0 has no direction, in the reference as here) the entry must be NaN too."""
    dev = np.asarray(dev)
    with np.errstate(invalid="ignore"):
        x = excess(dev, ref, E)
    both_nan = np.isnan(np.asarray(ref, dtype=np.float64)) & np.isnan(dev.astype(np.float64))
    return ~((x <= 1.0) | both_nan)


def report(dev, ref, E, label):
    """'' if every entry is inside its bound, else a message naming the worst entry"""
    dev = np.asarray(dev)
    if not dev.size:
        return ""
    x = excess(dev, ref, E)
    bad = outside(dev, ref, E)
    if not bad.any():
        return ""
    k = np.unravel_index(int(np.argmax(np.where(np.isnan(x), np.inf, x))), x.shape)
    return "%s: %d of %d entries outside C E (C = %g); worst at %s: dev %r ref %r E %.3e (|err| / tolerance %.3g)" % (
        label, int(bad.sum()), x.size, C, k, float(dev[k]), float(ref[k]), float(np.asarray(E)[k]), float(x[k]))


# ==================================================================================================================
# the passes as the tests run them
# ==================================================================================================================
PASSES = {
    "drift": dict(strength=1e-3, angle_strength=2e-3, std=0.2, dir=(0.3, -0.5, 0.8), seed=42),
    "drift_normalized": dict(strength=1e-4, angle_strength=2e-3, std=0.2, seed=7),
    "noise": dict(translation_std=0.1, rotation_std=0.1, point_std=0.1, seed=99),
    "sin": dict(dir=(1.0, 0.7, -0.4), noise_dir=(0.3, 2.0, -1.0), strength=1.5, frequency=2.0),
}


def evaluate(kind, cams15, pts, rec, prm, u=U, mutations=(), reference=True, oracle=False):
    """One pass over (cams15, pts) with the statistics record rec (20 f64: the kernels' argument) and parameters prm:
    dict(ref_c, ref_p (longdouble, None unless reference), c, Ec, p, Ep (the restated kernel of unit roundoff u)).
    oracle: the bound for the CPU oracle's libm draws (DRAW_ABS) instead of the device's."""
    n_cam, n_pts = len(cams15), len(pts)
    if kind in ("drift", "drift_normalized"):
        zc, zp = drift_draws(prm["seed"], n_cam, n_pts)
        common = (cams15, pts, rec[15:18], prm["strength"], prm["angle_strength"], prm["std"])
        if kind == "drift":
            ref = drift(*common, prm["dir"], zc, zp)[:2] if reference else (None, None)
            out = k_add_drift(*common, prm["dir"], zc, zp, u=u, mutations=mutations, oracle=oracle)
        else:
            ref = drift_normalized(*common, zc, zp, rec[3:6])[:2] if reference else (None, None)
            out = k_add_drift(*common, None, zc, zp, u=u, std3=rec[3:6], mutations=mutations, oracle=oracle)
    elif kind == "noise":
        zc, zp = noise_draws(prm["seed"], n_cam, n_pts)
        args = (cams15, pts, rec[19], prm["translation_std"], prm["rotation_std"], prm["point_std"], zc, zp)
        ref = noise_entities(*args) if reference else (None, None)
        out = k_add_noise_entities(*args, u=u, mutations=mutations, oracle=oracle)
    elif kind == "sin":
        args = (cams15, pts, rec[12:15], prm["dir"], prm["noise_dir"], prm["strength"], prm["frequency"])
        ref = sin_noise(*args) if reference else (None, None)
        out = k_add_sin_noise(*args, u=u, mutations=mutations)
    else:
        raise AssertionError(kind)
    return dict(ref_c=ref[0], ref_p=ref[1], c=out[0], Ec=out[1], p=out[2], Ep=out[3])


def resolved(E, scale):
    """True where a bound says something about a quantity of that scale: C E below it"""
    return C * np.asarray(E, dtype=np.float64) < scale


# the runs of tests/test_gpu_f32.py on grid_cameras_points(3, cpb=10, ppb=20, L=5.0): (kind, parameters, the factor of
# max(1, max |cameras|) that file used to allow on every camera entry (None: it had no camera check), the factor of
# max |points| on every point entry)
F32_FILE_RUNS = (
    ("drift", dict(strength=1e-3, angle_strength=2e-3, std=0.2, dir=(0.3, -0.5, 0.8), seed=42), 4e-6, 4e-6),
    ("noise", dict(translation_std=0.1, rotation_std=0.1, point_std=0.1, seed=99), 1e-5, 4e-6),
    ("drift_normalized", dict(strength=0.01, angle_strength=0.01, std=0.1, seed=7), None, 2e-5),
    ("sin", dict(dir=(1.0, 1.0, 0.0), noise_dir=(0.0, 1.0, 0.0), strength=1.0, frequency=2.0), 1e-5, 1e-5),
)


def f32_old_bounds(r, old_c, old_p):
    """(old camera bound or None, old point bound) of an evaluation r: the global bounds scaled by the largest entry"""
    mc = max(1.0, float(np.abs(r["ref_c"]).max())) if len(r["ref_c"]) else 1.0
    return (None if old_c is None else old_c * mc), old_p * float(np.abs(r["ref_p"]).max())
