"""References for the error sums sum |du|^norm + |dv|^norm (k_observations<MODE_ERROR | MODE_ERROR12 | MODE_NOISE_ERROR12>,
k_residual_jacobian_l<.., WITH_ERR>, ticket_fold_n) -- test helper, shared by tests/test_errref.py (CPU) and
tests/test_gpu_error_sums_reference.py.

Three references, each judged on the CPU by tests/test_errref.py before the device is held to it:

  * EXACT scenes (scene()): every quantity is chosen so that the device's arithmetic is exact.  R = I, k1 = k2 = 0, f in
    {0.5, 1, 2}, t = (c + 1, 3 c, 0) for camera c, points (x, y, -2^e) with integer x, y in +-2^9 and e in {0, 1, 2}.  The
    projection is f / 2^e (x + c + 1, y + 3 c): a dyadic number with at most three fractional bits.  The observed pixel is
    f / 2^e (x + c + 1 - g q_u, y + 3 c - g q_v) with g = max(1, 2^e / f) and integers q in +-64 hashed from (observation,
    camera, point): the residual is then the INTEGER s q, s = max(1, f / 2^e) in {1, 2}.  (With an observed integer taken
    freely in +-2^10 the residual f / 2^e (..) would be a multiple of 1/8, not an integer: g makes it one.  The observed
    integer is x + c + 1 - g q: inside +-2^10 + c.)  sum |a| and sum a^2 are integers below 2^53, every partial sum of
    either is an integer below 2^53 too, so EVERY summation order gives the same bits and a Python int is the reference.
    Layouts: "one" (one camera), "rows" (camera-major rows of the dome's lengths, with runs of empty rows inside a tile),
    "singles" (one observation per camera: more than kCamW = 12 cameras per wave, the slow path on sorted input),
    "permuted" (the rows layout's observations in a random order: cam_idx forms only).

  * one TERM: |a|^y in np.longdouble (term_ref; agreement with mpmath to 2^-60 is asserted on the CPU), and the bound
        E(a, y) = C (|y ln a| + 1) 2^-53 |a|^y
    -- the form of the kernels' contract "relative error ~ |y ln a| ulps": the logarithm's rounding error, about an ulp of
    |ln a|, is multiplied by y in the exponent, and the exponential adds its own ulp.  C is not chosen: it is twice the
    worst |pow_tab - reference| / (E / C) that the EXACT restatement of pow_tab below (pow_tab_exact: m2log_tab with its
    signed k, exp_tab, every FMA as float(Fraction) = one rounding) reaches over pow_sample(); tests/test_errref.py
    measures that ratio, asserts it is at most C / 2 and that C is not more than a tenth above twice the measurement.

  * a SUM of n terms t_i accumulated by a launch of a given shape:
        sum_i E_i + depth(n, shape) 2^-53 sum_i t_i + 2^-60 sum_i t_i
    (all terms are >= 0, so every partial sum is at most the total and each of the `depth` additions on the longest path
    rounds by at most 2^-53 of it; the last summand is the long-double reference's own accumulation error).  device_depth
    counts that path from kernels.hpp:
        lane          2 OPL       per tile one addition joins |du|^y and |dv|^y, one adds the pair to the lane's sum
        wave tree     6           wave_sum's shuffle levels
        workgroup     WPB         thread 0 adds the waves' values one after the other
        last arriver  P + 2       a thread's P = ceil(G / (64 WPB)) partials (four chains: at most P additions on one),
                                  then (a0 + a1) + (a2 + a3)
                      6 + WPB     its wave tree and its waves in order
    with G = ceil(ceil(n / 64) / (WPB OPL)) workgroups; the light passes launch WPB = 8, OPL = 3, the fused Jacobian
    WPB = 16, OPL = 1 below 6 000 000 observations (capi.hip: launch_obs, jacobian_shape)."""
import math
import os
import re
import struct
from fractions import Fraction

import numpy as np

from _problems import DOME_LENGTHS

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise RuntimeError("tests/_errref.py needs an extended long double (64-bit mantissa); this platform's np.longdouble has "
                       "%d mantissa bits" % np.finfo(LD).nmant)

U = 2.0 ** -53
C = 4.3                    # twice the worst ratio of the exact restatement over pow_sample(), 2.137 (measured; tests/test_errref.py)
NORMS = (0.1, 0.5, 1.25, 1.5, 3.0, 4.0, 7.3, 30.0)
LIGHT_SHAPE = (8, 3)       # (waves per workgroup, tiles of 64 observations per wave): k_observations as launch_obs launches it
JAC_SHAPE = (16, 1)        # k_residual_jacobian_l below kJacOneTileBelow observations
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "city2ba_amd", "csrc", "noise_tables.inc")


# ==================================================================================================================
# exact-integer scenes
# ==================================================================================================================
N_PTS = 4099                                                # a prime: the point of an observation does not repeat with the tile
LAYOUTS = ("one", "rows", "singles", "permuted")


def _row_lengths(n):
    """the dome's row lengths in order, again and again until they hold n observations (the last row cut), with a run of
    three empty rows behind every row whose length is odd: empty rows at the start, inside tiles and in runs"""
    out, left, k = [], n, 0
    while left > 0:
        length = min(int(DOME_LENGTHS[k % len(DOME_LENGTHS)]), left)
        out.append(length)
        if length % 2:
            out += [0, 0, 0]
        left -= length
        k += 1
    return np.asarray(out, dtype=np.int64)


def scene(n, layout="one", seed=0):
    """dict(cams15 [n_cam, 15], pts [N_PTS, 3], row_ptr (int64 [n_cam + 1]; None for "permuted"), cam_idx, pt_idx (int64 [n]),
    uv, proj [n, 2] (f64: the observed pixel and the exact projection), a [n, 2] (int64: the residual proj - uv))"""
    assert layout in LAYOUTS
    o = np.arange(n, dtype=np.int64)
    if layout == "one":
        counts = np.asarray([n], dtype=np.int64)
    elif layout == "singles":
        counts = np.ones(n, dtype=np.int64)
    else:
        counts = _row_lengths(n)
    n_cam = len(counts)
    cam = np.repeat(np.arange(n_cam, dtype=np.int64), counts)
    assert len(cam) == n
    pt = (7 * o + 3) % N_PTS
    if layout == "permuted":
        order = np.random.default_rng(seed + 77).permutation(n)
        cam, pt = cam[order], pt[order]
    j = np.arange(N_PTS, dtype=np.int64)
    x, y, e = (j * 389) % 1025 - 512, (j * 211 + 57) % 1025 - 512, j % 3
    pts = np.column_stack([x, y, -(2 ** e)]).astype(np.float64)
    c = np.arange(n_cam, dtype=np.int64)
    f = np.asarray([0.5, 1.0, 2.0])[c % 3]
    cams15 = np.zeros((n_cam, 15))
    cams15[:, [0, 4, 8]] = 1.0
    cams15[:, 9], cams15[:, 10], cams15[:, 12] = c + 1, 3 * c, f
    scale = f[cam] / (2.0 ** e[pt])                            # f / 2^e in {1/8 .. 2}: exact
    s = np.maximum(1.0, scale).astype(np.int64)                # 1 or 2
    g = np.maximum(1.0, 1.0 / scale).astype(np.int64)          # 1, 2, 4 or 8
    q = np.column_stack([(31 * o + 17 * cam + 13 * pt) % 129 - 64, (37 * o + 11 * cam + 29 * pt + 5) % 129 - 64])
    world = np.column_stack([x[pt] + cam + 1, y[pt] + 3 * cam])
    proj = world * scale[:, None]
    uv = (world - g[:, None] * q) * scale[:, None]
    a = q * s[:, None]
    row_ptr = None if layout == "permuted" else np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return dict(cams15=cams15, pts=pts, row_ptr=row_ptr, cam_idx=cam, pt_idx=pt, uv=uv, proj=proj, a=a, n_cam=n_cam)


def exact_sums(a):
    """(sum |a|, sum a^2) over the residuals a [n, 2] as Python ints"""
    a = np.asarray(a, dtype=np.int64)
    return int(np.abs(a).sum()), int((a * a).sum())


def exact_prefix_sums(a):
    """(S1, S2): S[k] = the sums over the first k observations (int64 arrays of length n + 1; exact: far below 2^63)"""
    a = np.asarray(a, dtype=np.int64)
    z = np.zeros(1, dtype=np.int64)
    return (np.concatenate([z, np.cumsum(np.abs(a).sum(axis=1))]), np.concatenate([z, np.cumsum((a * a).sum(axis=1))]))


# ==================================================================================================================
# one term: the long-double power, its bound, the exact restatement of pow_tab
# ==================================================================================================================
def term_ref(a, y):
    """|a|^y in long double (a: f64 array or scalar, y: the f64 exponent)"""
    with np.errstate(over="ignore", under="ignore"):
        return np.power(np.abs(np.asarray(a, dtype=np.float64)).astype(LD), LD(np.float64(y)))


def term_weight(a, y):
    """(|y ln a| + 1) 2^-53 |a|^y as f64: E / C.  0 for a = 0."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        ln = np.where(a > 0, np.abs(np.log(np.where(a > 0, a, 1.0).astype(LD))), LD(0))
        return ((np.float64(y) * ln + 1) * LD(U) * term_ref(a, y)).astype(np.float64)


def term_bound(a, y):
    return C * term_weight(a, y)


def value_class(v):
    """'zero' / 'subnormal' / 'inf' / 'nan' / 'normal' of a double"""
    v = float(v)
    if v != v:
        return "nan"
    if v == 0.0:
        return "zero"
    if math.isinf(v):
        return "inf"
    return "subnormal" if abs(v) < 2.0 ** -1022 else "normal"


_TABLE = None


def table():
    """noise_tables.inc as [704, 2] doubles (entries [512, 640): (1 / c, -2 ln c); [640, 704): 2^(j / 128), 128 doubles)"""
    global _TABLE
    if _TABLE is None:
        rows = re.findall(r"^\{(\S+), (\S+)\},$", open(INC).read(), flags=re.M)
        _TABLE = np.array([[float.fromhex(p), float.fromhex(q)] for p, q in rows])
        assert _TABLE.shape == (704, 2)
    return _TABLE


def _fma(p, q, r):
    """fma(p, q, r): the exact value rounded once (float(Fraction) rounds to nearest, ties to even)"""
    return float(Fraction(p) * Fraction(q) + Fraction(r))


LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
EXP_INV, EXP_HI, EXP_LO = float.fromhex("0x1.71547652b82fep+7"), float.fromhex("0x1.62e42fee00000p-8"), float.fromhex("0x1.a39ef35793c76p-40")


def m2log_split(x):
    """(z, k, i) of m2log_tab: x = z 2^k with z in [0.6875, 1.375), k SIGNED (the arithmetic shift of the 32-bit word), and z's
    table interval"""
    bits = struct.unpack("<Q", struct.pack("<d", x))[0]
    hi, lo = bits >> 32, bits & 0xFFFFFFFF
    tmp = (hi - 0x3FE60000) & 0xFFFFFFFF
    i = (tmp >> 13) & 127
    k = tmp >> 20
    k = k - 4096 if k >= 2048 else k
    zhi = (hi - (tmp & 0xFFF00000)) & 0xFFFFFFFF
    z = struct.unpack("<d", struct.pack("<Q", (zhi << 32) | lo))[0]
    return z, k, i


MUTATIONS = ("coef", "no_kd_tail")     # -2/3 shortened to -0.6667; kd dropped from `tail` (tests/test_errref.py: both leave E)


def m2log_tab_exact(x, mutation=None):
    """camera_math.hpp: m2log_tab, operation for operation, for a normal x > 0"""
    z, k, i = m2log_split(x)
    invc, m2logc = (float(v) for v in table()[512 + i])
    r, kd = _fma(z, invc, -1.0), float(k)
    p = _fma(r, -2.0 / 7.0, 1.0 / 3.0)
    p = _fma(r, p, -2.0 / 5.0)
    p = _fma(r, p, 0.5)
    p = _fma(r, p, -0.6667 if mutation == "coef" else -2.0 / 3.0)
    p = _fma(r, p, 1.0)
    head = _fma(kd, -2.0 * LN2_HI, m2logc)
    tail = -2.0 * r if mutation == "no_kd_tail" else _fma(kd, -2.0 * LN2_LO, -2.0 * r)
    return head + _fma(r * r, p, tail)


def exp_tab_exact(x):
    """camera_math.hpp: exp_tab, operation for operation, for |x| < 700"""
    kf = float(round(x * EXP_INV))                           # rint: to nearest, ties to even -- Python's round() of a float
    r = _fma(-kf, EXP_HI, x)
    r = _fma(-kf, EXP_LO, r)
    ki = int(kf)
    T = float(table()[640:].reshape(-1)[ki & 127])
    q = _fma(r, 1.0 / 120.0, 1.0 / 24.0)
    q = _fma(r, q, 1.0 / 6.0)
    q = _fma(r, q, 0.5)
    p = _fma(r * r, q, r)
    return math.ldexp(_fma(T, p, T), ki >> 7)                # |x| < 600 here: the result is a normal number, ldexp is exact


def pow_tab_fallback(a, y):
    """True when pow_tab hands (a, y) to the library's pow: a outside (2^-1000, 2^1000), or |y ln a| (as the kernel computes it) >= 600"""
    a, y = float(a), float(y)
    if not (a > 2.0 ** -1000 and a < 2.0 ** 1000):
        return True
    l = (-0.5 * y) * m2log_tab_exact(a)
    return not (l > -600.0 and l < 600.0)


def pow_tab_exact(a, y, mutation=None):
    """the bits pow_tab(a, y) returns on its table route; None where it takes the library's pow"""
    a, y = float(a), float(y)
    if pow_tab_fallback(a, y):
        return None
    return exp_tab_exact((-0.5 * y) * m2log_tab_exact(a, mutation))


def _from_hi_lo(hi, lo):
    return struct.unpack("<d", struct.pack("<Q", (hi << 32) | lo))[0]


def pow_sample(seed=3):
    """[(a, y, tag)]: the arguments the term tests run, per norm of NORMS:
         sizes   300 residual sizes log-uniform in 1e-12 .. 1e3
         near1   100 arguments within 0.02 of 1, both neighbours of 1.0, 1 +- 2^-30, 1.0 itself
         ends    both ends of up to 12 table intervals of z (at k = 0 and at one other exponent), z = 0.6875 and z = 1.375
         exps    2^+-500, 2^+-900, 2^+-990, 1.5 2^+-999 (the table route for small y, the library's pow for the rest), the first
                 arguments outside (2^-1000, 2^1000), and 2^-700
         edge    |y ln a| = 599.9 and 600.1 from both sides, where such an a is a finite double
    about 3 700 pairs in all"""
    rng = np.random.default_rng(seed)
    out = []
    for y in NORMS:
        out += [(float(10.0 ** v), y, "sizes") for v in rng.uniform(-12.0, 3.0, 300)]
        out += [(float(v), y, "near1") for v in rng.uniform(0.98, 1.02, 100)]
        out += [(v, y, "near1") for v in (1.0, math.nextafter(1.0, 0.0), math.nextafter(1.0, 2.0), 1.0 - 2.0 ** -30, 1.0 + 2.0 ** -30)]
        for i in sorted({0, 1, 78, 79, 80, 81, 127} | {int(v) for v in rng.integers(0, 128, 5)}):
            hi = 0x3FE60000 + (i << 13)
            for k in (0, int(rng.integers(-40, 11))):
                out += [(math.ldexp(_from_hi_lo(hi, 0), k), y, "ends"), (math.ldexp(_from_hi_lo(hi + 0x1FFF, 0xFFFFFFFF), k), y, "ends")]
        out += [(0.6875, y, "ends"), (1.375, y, "ends")]
        for ex in (500, 900, 990):
            out += [(2.0 ** ex, y, "exps"), (2.0 ** -ex, y, "exps")]
        out += [(1.5 * 2.0 ** 999, y, "exps"), (1.5 * 2.0 ** -999, y, "exps"), (2.0 ** 1000, y, "exps"), (2.0 ** -1000, y, "exps"),
                (math.nextafter(2.0 ** 1000, 0.0), y, "exps"), (math.nextafter(2.0 ** -1000, 1.0), y, "exps"), (2.0 ** -700, y, "exps")]
        for l in (599.9, 600.1, -599.9, -600.1):
            if abs(l / y) < 690.0:
                out.append((math.exp(l / y), y, "edge"))
    return out


def restatement_ratio(a, y, mutation=None):
    """|pow_tab_exact - reference| / ((|y ln a| + 1) 2^-53 |a|^y); None on the fallback route"""
    v = pow_tab_exact(a, y, mutation)
    if v is None:
        return None
    return float(abs(LD(v) - term_ref(a, y)) / LD(term_weight(a, y)))


# ==================================================================================================================
# sums
# ==================================================================================================================
def launch_grid(n, shape):
    wpb, opl = shape
    return max(1, -(-(-(-int(n) // 64)) // (wpb * opl)))


def device_depth(n, shape=LIGHT_SHAPE):
    """additions on the longest path from a term to the launch's sum (module docstring)"""
    wpb, opl = shape
    per_thread = -(-launch_grid(n, shape) // (64 * wpb))
    return 2 * opl + 6 + wpb + (per_thread + 2) + 6 + wpb


def sum_ref(res, y):
    """(reference sum (long double), sum of the term bounds E_i, sum of the terms (f64)) of the residuals res [n, 2] (f64)"""
    t = term_ref(np.asarray(res, dtype=np.float64).reshape(-1), y)
    total = t.sum()
    return total, float(term_bound(np.asarray(res, dtype=np.float64).reshape(-1), y).sum()), float(total)


def sum_bound(res, y, shape=LIGHT_SHAPE):
    """(reference, bound): |dev - reference| <= bound for a correct launch of that shape over the residuals res [n, 2]"""
    total, e_terms, t = sum_ref(res, y)
    n = np.asarray(res).reshape(-1, 2).shape[0]
    return total, e_terms + device_depth(n, shape) * U * t + 2.0 ** -60 * t
