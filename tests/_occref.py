"""Exact-geometry reference for the occlusion rays of the mesh generator (k_occlusion, k_occlusion_bvh and the host
hierarchy of csrc/host_bvh.hpp), and the ray families the tests run (test helper; shared by tests/test_occref.py,
tests/test_gpu_occlusion_reference.py, tests/test_gpu_generate.py).  Same conventions as tests/_jacref.py and
tests/_noiseref.py, whose LD and C it takes.

Five parts:
  * rays(): the float32 ray (o, d, tfar) of an observation exactly as both kernels and the C oracle form it.
  * the float32 restatement (restate(), occluded_numpy(), mt_hit(), box_hit()): the kernels' triangle test and slab test
    in numpy float32, operation by operation (no contraction: the library is compiled with -ffp-contract=off), on
    (v0, e1, e2) rows whose edges were subtracted in float32, as the all-triangles kernel forms them in registers and the
    hierarchy's slots hold them.  restate() carries beside det, u, w, u + w and th a first-order running bound E
    (u = 2^-24): every rounded operation adds u |result| to the propagated error of its operands; 1 / det takes the
    rigorous form E_det / (|det| (|det| - E_det)) and is unbounded where E_det reaches |det|.
  * exact(): the same five quantities in np.longdouble from the float32 ray and the float32 rows (the real-number
    value of the formula on the numbers the kernels are given).  Each of the seven comparisons that fix a pair's outcome
    (det != 0, u >= 0, u <= 1, w >= 0, u + w <= 1, th > 0, th <= tfar) is a sign test on numerators; where a
    numerator is below THIN = 2^-40 of the sum of the magnitudes of its terms the sign is taken again in
    fractions.Fraction, without a division, so the outcome is exact.
  * judge(): a comparison is DECIDED when its exact value is further from its threshold than C E; nothing of a pair is
    decided unless det != 0 is.  A pair is a decided hit when all seven are decided and pass, a decided miss when one
    decided comparison fails.  A ray is decided occluded if some triangle is a decided hit, decided clear if every
    triangle is a decided miss, open otherwise.  On a decided ray float32 arithmetic in the kernels' order cannot
    answer differently; on an open ray the test holds the device only to the restatement, bit for bit.
  * closed_exact(): the answer of the geometry itself, for the union of closed coplanar polygons (a ray through a
    shared edge or vertex is occluded in fact although each triangle alone may be open).  A device `keep` on a ray
    closed_exact() calls occluded is a LEAK; the tests count leaks and require every one to be an open ray.

The families (family(name)) are lists of cases; a case is a cross product of cameras and points over one mesh, with the
rays in camera-major order (the order Level 1 emits them).  Cameras look along an axis (signed permutation matrices),
so their centres are exact in every code path and the tiny focal length makes the predicate of Level 1 pass every
point in front of a camera."""
import ctypes as C_
import functools
from fractions import Fraction

import numpy as np

from _jacref import LD, C

f32 = np.float32
f64 = np.float64
U32 = 2.0 ** -24            # unit roundoff of f32
THIN = 2.0 ** -40           # below this share of its terms' magnitude a long-double numerator is re-evaluated exactly
K_OCC_TILE = 256            # kernels.hpp: kOccTile
K_BLOCK = 256               # kernels.hpp: kBlock
K_BVH_MIN = 64              # kernels.hpp: kBvhMinTriangles
EMPTY = -2 ** 31
CMP = ("det != 0", "u >= 0", "u <= 1", "w >= 0", "u + w <= 1", "th > 0", "th <= tfar")
PAIR_CHUNK = 1 << 19        # (ray, triangle) pairs evaluated at a time


# ==================================================================================================================
# the ray
# ==================================================================================================================
def rays(centers, pts):
    """(o, d, tfar) float32 of the rays centre -> point, [n, 3], [n, 3], [n]: e = p - c, mag = sqrt((ex ex + ey ey) +
    ez ez), inv = 1 / mag in float64; o = (float)c, d = (float)(e inv), tfar = (float)mag - 1e-6f"""
    c = np.asarray(centers, dtype=f64).reshape(-1, 3)
    p = np.asarray(pts, dtype=f64).reshape(-1, 3)
    e = p - c
    with np.errstate(all="ignore"):
        mag = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        inv = 1.0 / mag
        d = (e * inv[:, None]).astype(f32)
    return c.astype(f32), d, mag.astype(f32) - f32(1e-6)


def ray_lengths(centers, pts):
    """|dir| in float64 as rays() forms it"""
    e = np.asarray(pts, dtype=f64).reshape(-1, 3) - np.asarray(centers, dtype=f64).reshape(-1, 3)
    return np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])


def slots_of(tri9):
    """[n, 9] rows (v0, e1, e2) with the edges subtracted in float32"""
    t = np.ascontiguousarray(tri9, dtype=f32).reshape(-1, 9)
    return np.concatenate([t[:, 0:3], t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3]], axis=1)


# ==================================================================================================================
# float32 restatement with its running bound
# ==================================================================================================================
class V:
    """a float32 value and the first-order bound of its distance from the real-number value"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = v, e

    def _r(self, v, e):
        return V(v, e + U32 * np.abs(v).astype(f64))

    def __mul__(self, o):
        return self._r(self.v * o.v, np.abs(self.v).astype(f64) * o.e + np.abs(o.v).astype(f64) * self.e)

    def __add__(self, o):
        return self._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return self._r(self.v - o.v, self.e + o.e)

    def inverse(self):
        a = np.abs(self.v).astype(f64)
        v = f32(1.0) / self.v
        room = a - self.e
        e = np.where(room > 0, self.e / (a * np.where(room > 0, room, 1.0)), np.inf)
        return self._r(v, e)


def restate(o, d, tfar, slots, bound=False):
    """the kernels' triangle test on every (ray, row) pair, float32: dict of det, u, w, uw, th [R, T] and hit (bool);
    with bound=True also E_det, E_u, E_w, E_uw, E_th (float64; inf where nothing can be said)"""
    o, d, slots = np.asarray(o, f32), np.asarray(d, f32), np.asarray(slots, f32)
    tfar = np.asarray(tfar, f32)[:, None]
    X = (lambda a: V(a)) if bound else (lambda a: a)
    ox, oy, oz = (X(o[:, k, None]) for k in range(3))
    dx, dy, dz = (X(d[:, k, None]) for k in range(3))
    v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z = (X(slots[None, :, k]) for k in range(9))
    with np.errstate(all="ignore"):
        px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
        det = (e1x * px + e1y * py) + e1z * pz
        idet = det.inverse() if bound else f32(1.0) / det
        tx, ty, tz = ox - v0x, oy - v0y, oz - v0z
        u = ((tx * px + ty * py) + tz * pz) * idet
        qx, qy, qz = ty * e1z - tz * e1y, tz * e1x - tx * e1z, tx * e1y - ty * e1x
        w = ((dx * qx + dy * qy) + dz * qz) * idet
        th = ((e2x * qx + e2y * qy) + e2z * qz) * idet
        uw = u + w
        val = (lambda a: a.v) if bound else (lambda a: a)
        r = {"det": val(det), "u": val(u), "w": val(w), "uw": val(uw), "th": val(th)}
        r["hit"] = ((r["det"] != 0) & ~(r["u"] < 0) & ~(r["u"] > 1) & ~(r["w"] < 0) & ~(r["uw"] > 1) & (r["th"] > 0)
                    & (r["th"] <= tfar))
        if bound:
            for k, a in (("det", det), ("u", u), ("w", w), ("uw", uw), ("th", th)):
                e = np.broadcast_to(np.asarray(a.e, dtype=f64), r[k].shape)
                r["E_" + k] = np.where(np.isfinite(e), e, np.inf)
    return r


def _chunks(n_rays, n_tri):
    step = max(1, PAIR_CHUNK // max(1, n_tri))
    return [(a, min(n_rays, a + step)) for a in range(0, n_rays, step)]


def hits_f32(o, d, tfar, slots):
    """[R, T] bool: the pairs the float32 test accepts"""
    out = np.zeros((len(o), len(slots)), dtype=bool)
    for a, b in _chunks(len(o), len(slots)):
        out[a:b] = restate(o[a:b], d[a:b], tfar[a:b], slots)["hit"]
    return out


def occluded_numpy(centers, pts, tri):
    """float32 rays as embree_rs::Ray::new(center as f32, dir.normalize() as f32), tfar = |dir| as f32 - 1e-6
    (src/generate.rs:456-464); occluded iff some triangle is hit with 0 < t <= tfar.  Same operation order as the
    kernel, numpy float32 arithmetic (no fused multiply-add)."""
    o, d, tfar = rays(centers, pts)
    tri = np.asarray(tri, dtype=f32).reshape(-1, 9)
    if not len(tri):
        return np.zeros(len(o), dtype=bool)
    return hits_f32(o, d, tfar, slots_of(tri)).any(axis=1)


def mt_hit(o, d, tfar, slots):
    """vectorised form of tests/test_bvh_host.py's mt_hit: ray i against row i (arrays of equal length)"""
    o, d, slots, tfar = np.asarray(o, f32), np.asarray(d, f32), np.asarray(slots, f32), np.asarray(tfar, f32)
    v0, e1, e2 = slots[:, 0:3], slots[:, 3:6], slots[:, 6:9]
    with np.errstate(all="ignore"):
        px = d[:, 1] * e2[:, 2] - d[:, 2] * e2[:, 1]
        py = d[:, 2] * e2[:, 0] - d[:, 0] * e2[:, 2]
        pz = d[:, 0] * e2[:, 1] - d[:, 1] * e2[:, 0]
        det = (e1[:, 0] * px + e1[:, 1] * py) + e1[:, 2] * pz
        idet = f32(1.0) / det
        tx, ty, tz = o[:, 0] - v0[:, 0], o[:, 1] - v0[:, 1], o[:, 2] - v0[:, 2]
        u = ((tx * px + ty * py) + tz * pz) * idet
        qx = ty * e1[:, 2] - tz * e1[:, 1]
        qy = tz * e1[:, 0] - tx * e1[:, 2]
        qz = tx * e1[:, 1] - ty * e1[:, 0]
        w = ((d[:, 0] * qx + d[:, 1] * qy) + d[:, 2] * qz) * idet
        th = ((e2[:, 0] * qx + e2[:, 1] * qy) + e2[:, 2] * qz) * idet
        return (det != 0) & ~(u < 0) & ~(u > 1) & ~(w < 0) & ~(u + w > 1) & (th > 0) & (th <= tfar)


def box_tn_tf(lo, hi, o, inv):
    """the slab test's (tn, tf) as the device's bvh_box_hit forms them; fmin / fmax drop a NaN operand ((lo - o) inf with
    lo == o).  Arrays [..., 3]."""
    with np.errstate(all="ignore"):
        a, b = (lo - o) * inv, (hi - o) * inv
        mn, mx = np.fmin(a, b), np.fmax(a, b)
        tn = np.fmax(np.fmax(mn[..., 0], mn[..., 1]), mn[..., 2])
        tf = np.fmin(np.fmin(mx[..., 0], mx[..., 1]), mx[..., 2])
    return tn, tf


def box_hit(lo, hi, o, inv, tfar):
    """vectorised form of tests/test_bvh_host.py's box_hit (float32 throughout)"""
    tn, tf = box_tn_tf(np.asarray(lo, f32), np.asarray(hi, f32), np.asarray(o, f32), np.asarray(inv, f32))
    with np.errstate(all="ignore"):
        return (tn <= tf * f32(1.00001) + f32(1e-30)) & (tf >= 0) & (tn <= np.asarray(tfar, f32) * f32(1.00001))


# ==================================================================================================================
# exact values and exact outcomes
# ==================================================================================================================
def _fraction_signs(o, d, tfar, slot):
    """the seven outcomes of one pair in exact rational arithmetic, by sign tests (no division)"""
    F = Fraction
    o, d = [F(float(x)) for x in o], [F(float(x)) for x in d]
    v0, e1, e2 = ([F(float(x)) for x in slot[3 * k:3 * k + 3]] for k in range(3))
    tf_ = F(float(tfar))
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    p = cross(d, e2)
    det = dot(e1, p)
    if det == 0:
        return (False,) * 7
    s = 1 if det > 0 else -1
    t = [o[k] - v0[k] for k in range(3)]
    q = cross(t, e1)
    nu, nw, nt = dot(t, p), dot(d, q), dot(e2, q)
    return (True, s * nu >= 0, s * (nu - det) <= 0, s * nw >= 0, s * (nu + nw - det) <= 0, s * nt > 0,
            s * (nt - tf_ * det) <= 0)


def exact(o, d, tfar, slots):
    """det, u, w, uw, th [R, T] in long double from the float32 ray and rows; cmp [7, R, T]: the exact outcome of each
    comparison of CMP (all False where det == 0); hit = all of them; thin = the number of pairs settled in Fraction"""
    o32, d32, s32, t32 = np.asarray(o, f32), np.asarray(d, f32), np.asarray(slots, f32), np.asarray(tfar, f32)
    o, d, slots = o32.astype(LD), d32.astype(LD), s32.astype(LD)
    tf_ = t32.astype(LD)[:, None]
    ox, oy, oz = (o[:, k, None] for k in range(3))
    dx, dy, dz = (d[:, k, None] for k in range(3))
    v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z = (slots[None, :, k] for k in range(9))
    A = np.abs
    with np.errstate(all="ignore"):
        px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
        apx, apy, apz = A(dy * e2z) + A(dz * e2y), A(dz * e2x) + A(dx * e2z), A(dx * e2y) + A(dy * e2x)
        det = e1x * px + e1y * py + e1z * pz
        sdet = A(e1x) * apx + A(e1y) * apy + A(e1z) * apz
        tx, ty, tz = ox - v0x, oy - v0y, oz - v0z
        nu = tx * px + ty * py + tz * pz
        snu = A(tx) * apx + A(ty) * apy + A(tz) * apz
        qx, qy, qz = ty * e1z - tz * e1y, tz * e1x - tx * e1z, tx * e1y - ty * e1x
        aqx, aqy, aqz = A(ty * e1z) + A(tz * e1y), A(tz * e1x) + A(tx * e1z), A(tx * e1y) + A(ty * e1x)
        nw = dx * qx + dy * qy + dz * qz
        snw = A(dx) * aqx + A(dy) * aqy + A(dz) * aqz
        nt = e2x * qx + e2y * qy + e2z * qz
        snt = A(e2x) * aqx + A(e2y) * aqy + A(e2z) * aqz
        s = np.sign(det)
        num = [det, s * nu, s * (nu - det), s * nw, s * (nu + nw - det), s * nt, s * (nt - tf_ * det)]
        scl = [sdet, snu, snu + sdet, snw, snu + snw + sdet, snt, snt + tf_ * sdet]
        cmp = np.stack([num[0] != 0, num[1] >= 0, num[2] <= 0, num[3] >= 0, num[4] <= 0, num[5] > 0, num[6] <= 0])
        thin = np.zeros(det.shape, dtype=bool)
        for n_, s_ in zip(num, scl):
            thin |= A(n_) <= THIN * s_
        cmp[1:, ~cmp[0]] = False
        for r, t in zip(*np.nonzero(thin)):
            cmp[:, r, t] = _fraction_signs(o32[r], d32[r], t32[r], s32[t])
        res = {"det": det, "u": nu / det, "w": nw / det, "uw": (nu + nw) / det, "th": nt / det, "cmp": cmp,
               "hit": cmp.all(axis=0), "thin": int(thin.sum())}
    return res


def judge_pairs(o, d, tfar, slots):
    """per pair: f32 hit, exact hit, decided hit, decided miss, and the count of thin pairs"""
    f = restate(o, d, tfar, slots, bound=True)
    x = exact(o, d, tfar, slots)
    tf_ = np.asarray(tfar, f32).astype(LD)[:, None]
    with np.errstate(all="ignore"):
        marg = [abs(x["det"]), abs(x["u"]), abs(x["u"] - 1), abs(x["w"]), abs(x["uw"] - 1), abs(x["th"]),
                abs(x["th"] - tf_)]
        bnd = [f["E_det"], f["E_u"], f["E_u"], f["E_w"], f["E_uw"], f["E_th"], f["E_th"]]
        dec = np.stack([(m.astype(f64) > C * b) & np.isfinite(b) for m, b in zip(marg, bnd)])
        dec[1:] &= dec[0]
    dhit = (dec & x["cmp"]).all(axis=0)
    dmiss = dec[0] & (dec[1:] & ~x["cmp"][1:]).any(axis=0)
    return {"f32": f["hit"], "exact": x["hit"], "dhit": dhit, "dmiss": dmiss, "thin": x["thin"], "dec": dec, "cmp": x["cmp"]}


def judge(o, d, tfar, slots, own=None):
    """per ray: f32 (the restatement's occluded), exact (some triangle is met in exact arithmetic; exact_other: one that is not the ray's own), occluded / clear (decided), open, contradicted (decided pairs the
    restatement answers differently: must be 0), self_hit (the restatement accepts the ray's own triangle), thin"""
    n = len(o)
    out = {k: np.zeros(n, dtype=bool) for k in ("f32", "exact", "exact_other", "occluded", "clear", "self_hit")}
    out["contradicted"], out["thin"], out["hits"] = 0, 0, np.zeros((n, len(slots)), dtype=bool)
    for a, b in _chunks(n, len(slots)):
        j = judge_pairs(o[a:b], d[a:b], tfar[a:b], slots)
        out["f32"][a:b] = j["f32"].any(axis=1)
        out["exact"][a:b] = j["exact"].any(axis=1)
        out["occluded"][a:b] = j["dhit"].any(axis=1)
        out["clear"][a:b] = j["dmiss"].all(axis=1)
        out["hits"][a:b] = j["f32"]
        out["contradicted"] += int((j["dhit"] & ~j["f32"]).sum() + (j["dmiss"] & j["f32"]).sum()
                                   + (j["dhit"] & ~j["exact"]).sum() + (j["dmiss"] & j["exact"]).sum())
        out["thin"] += j["thin"]
        other = j["exact"].copy()
        if own is not None:
            ow = np.asarray(own[a:b])
            has = ow >= 0
            out["self_hit"][a:b][has] = j["f32"][np.nonzero(has)[0], ow[has]]
            other[np.nonzero(has)[0], ow[has]] = False
        out["exact_other"][a:b] = other.any(axis=1)
    out["open"] = ~out["occluded"] & ~out["clear"]
    return out


# ==================================================================================================================
# the geometry's own answer: closed coplanar polygons
# ==================================================================================================================
def _closed_fraction(o, d, tfar, poly):
    F = Fraction
    o, d = [F(float(x)) for x in o], [F(float(x)) for x in d]
    P = [[F(float(x)) for x in v] for v in poly]
    sub = lambda a, b: [a[0] - b[0], a[1] - b[1], a[2] - b[2]]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    n = cross(sub(P[1], P[0]), sub(P[2], P[0]))
    dn = dot(n, d)
    if dn == 0:
        return False
    t = dot(n, sub(P[0], o)) / dn
    if not (0 < t <= F(float(tfar))):
        return False
    x = [o[k] + t * d[k] for k in range(3)]
    sg = [dot(n, cross(sub(P[(i + 1) % len(P)], P[i]), sub(x, P[i]))) for i in range(len(P))]
    return all(s >= 0 for s in sg)


def closed_exact(o, d, tfar, polys):
    """[R] bool: the ray crosses, at 0 < t <= tfar, the closed convex planar polygon of some entry of `polys` (each
    [k, 3], float32 or float64 values, counter-clockwise about (v1 - v0) x (v2 - v0)).  float64 where the crossing is clear of every
    boundary by 1e-9 of the scale, Fraction otherwise.  A ray in a polygon's plane does not cross it."""
    o32, d32, t32 = np.asarray(o, f32), np.asarray(d, f32), np.asarray(tfar, f32)
    o, d, tf_ = o32.astype(f64), d32.astype(f64), t32.astype(f64)
    occ = np.zeros(len(o), dtype=bool)
    eps = 1e-9
    for poly in polys:
        P = np.asarray(poly, f64)
        n = np.cross(P[1] - P[0], P[2] - P[0])
        size = np.abs(P - P.mean(0)).max() + 1e-300
        nn = np.linalg.norm(n) + 1e-300
        with np.errstate(all="ignore"):
            dn = d @ n
            t = ((P[0] - o) @ n) / dn
            x = o + t[:, None] * d
            reach = np.abs(o - P[0]).max(axis=1) + size
            edge = np.stack([np.cross(P[(i + 1) % len(P)] - P[i], x - P[i]) @ n / (nn * size * size) for i in range(len(P))])
            tol = eps * reach * nn / np.maximum(np.abs(dn), 1e-300)             # a grazing ray's crossing is known less well
            inside, outside = (edge > tol / size).all(axis=0), (edge < -tol / size).any(axis=0)
            tin = (t > tol) & (t < tf_ - tol)
            tout = (t < -tol) | (t > tf_ + tol)
            clear_no = outside | tout
            clear_yes = inside & tin & np.isfinite(t)
        occ |= clear_yes
        for r in np.nonzero(~clear_yes & ~clear_no & ~occ)[0]:
            occ[r] = _closed_fraction(o32[r], d32[r], t32[r], P)
    return occ


# ==================================================================================================================
# the host hierarchy, read back through the C ABI and walked in numpy
# ==================================================================================================================
def bvh_build(tri):
    """(nodes [n, 16] f32, slots [n_tri, 12] f32, order [n_tri] u32, depth) of c2b_bvh_build"""
    from city2ba_amd import _lib as L
    tri = np.ascontiguousarray(tri, dtype=f32).reshape(-1, 9)
    h = C_.c_void_p()
    L.check(L.lib().c2b_bvh_build(tri.ctypes.data_as(C_.c_void_p), len(tri), C_.byref(h)))
    try:
        nn, ns, depth = C_.c_int64(), C_.c_int64(), C_.c_int()
        L.check(L.lib().c2b_bvh_sizes(h, C_.byref(nn), C_.byref(ns), C_.byref(depth)))
        nodes = np.zeros((nn.value, 16), dtype=f32)
        tris = np.zeros((max(ns.value, 1), 12), dtype=f32)
        order = np.zeros(ns.value, dtype=np.uint32)
        L.check(L.lib().c2b_bvh_copy(h, nodes.ctypes.data_as(C_.c_void_p), tris.ctypes.data_as(C_.c_void_p),
                                     order.ctypes.data_as(C_.c_void_p)))
    finally:
        L.lib().c2b_bvh_free(h)
    return nodes, tris[:ns.value], order, depth.value


def path_boxes(nodes, n_slots):
    """(lo [n_slots, D, 3], hi [n_slots, D, 3], used [n_slots, D]): the boxes a traversal must pass, root to leaf, to
    reach each slot"""
    paths = [None] * n_slots
    ints = nodes.view(np.int32)
    stack = [(0, [])]
    while stack:
        i, path = stack.pop()
        for side in range(2):
            c = int(ints[i, 12 + side])
            if c == EMPTY:
                continue
            here = path + [(nodes[i, 6 * side:6 * side + 3], nodes[i, 6 * side + 3:6 * side + 6])]
            if c >= 0:
                stack.append((c, here))
            else:
                v = ~c & 0xFFFFFFFF
                for s in range(v >> 3, (v >> 3) + (v & 7) + 1):
                    paths[s] = here
    assert all(p is not None for p in paths)
    D = max(len(p) for p in paths)
    lo, hi = np.zeros((n_slots, D, 3), f32), np.zeros((n_slots, D, 3), f32)
    used = np.zeros((n_slots, D), dtype=bool)
    for s, p in enumerate(paths):
        for k, (l, h) in enumerate(p):
            lo[s, k], hi[s, k], used[s, k] = l, h, True
    return lo, hi, used


def pruned_hits(o, d, tfar, nodes, slots):
    """over the (ray, slot) pairs the restatement accepts: how many the slab tests along the slot's path would prune, the
    number of accepted pairs, and the worst tn - tfar, in ulps of tfar, over every box of those paths"""
    lo, hi, used = path_boxes(nodes, len(slots))
    hits = hits_f32(o, d, tfar, slots[:, :9])
    r, s = np.nonzero(hits)
    if not len(r):
        return 0, 0, -np.inf
    with np.errstate(all="ignore"):
        inv = f32(1.0) / d[r]
        ok = box_hit(lo[s], hi[s], o[r][:, None, :], inv[:, None, :], tfar[r][:, None]) | ~used[s]
        tn, _ = box_tn_tf(lo[s], hi[s], o[r][:, None, :], inv[:, None, :])
        ulp = np.spacing(np.abs(tfar[r]))[:, None]
        over = np.where(used[s] & np.isfinite(tn), (tn.astype(f64) - tfar[r][:, None].astype(f64)) / ulp.astype(f64), -np.inf)
    return int((~ok.all(axis=1)).sum()), len(r), float(over.max())


def traverse(o, d, tfar, nodes, slots):
    """[R] bool: k_occlusion_bvh in numpy (all rays step together; a ray is occluded if any leaf it reaches hits)"""
    ints = nodes.view(np.int32)
    occ = np.zeros(len(o), dtype=bool)
    with np.errstate(all="ignore"):
        inv = f32(1.0) / d
    stack = [(0, np.arange(len(o)))]
    while stack:
        i, idx = stack.pop()
        idx = idx[~occ[idx]]
        for side in range(2):
            c = int(ints[i, 12 + side])
            if c == EMPTY or not len(idx):
                continue
            go = idx[box_hit(nodes[i, 6 * side:6 * side + 3], nodes[i, 6 * side + 3:6 * side + 6], o[idx], inv[idx], tfar[idx])]
            if c >= 0:
                stack.append((c, go))
            elif len(go):
                v = ~c & 0xFFFFFFFF
                for s in range(v >> 3, (v >> 3) + (v & 7) + 1):
                    occ[go] |= mt_hit(o[go], d[go], tfar[go], np.broadcast_to(slots[s, :9], (len(go), 9)))
    return occ


# ==================================================================================================================
# cameras and cases
# ==================================================================================================================
def cameras_for(centers, pts):
    """cams15 [n, 15] with the given centres, each looking along the signed axis that has most of `pts` in front of it
    (signed permutation matrices: R, t = -R c and the centre -R^-1 t are exact), focal 1e-6, no distortion: Level 1's
    predicate keeps exactly the points in front of a camera"""
    centers = np.asarray(centers, f64).reshape(-1, 3)
    cams = np.zeros((len(centers), 15))
    for i, c in enumerate(centers):
        e = np.asarray(pts, f64).reshape(-1, 3) - c
        best = max(((int((s * e[:, a] > 0).sum()), a, s) for a in range(3) for s in (1.0, -1.0)), key=lambda t: t[0])
        _, a, s = best
        fwd, up = np.zeros(3), np.zeros(3)
        fwd[a], up[(a + 1) % 3] = s, 1.0
        R = np.stack([np.cross(fwd, up), up, -fwd])                        # world -> camera, camera looks down -z
        cams[i, :9] = R.T.reshape(9)                                       # column-major
        cams[i, 9:12] = -(R @ c)
        cams[i, 12] = 1e-6
    return cams


class Case:
    """cameras x points over one mesh; ray r = (camera r // n_pts, point r % n_pts).  own[p]: the triangle point p lies on
    (-1: none).  marks: per-ray annotations of the family (aimed: ulps beside a seam, NaN where not aimed; far_face)."""

    def __init__(self, name, centers, pts, tri, own=None, polys=None, **marks):
        self.name = name
        self.centers = np.ascontiguousarray(centers, dtype=f64).reshape(-1, 3)
        self.pts = np.ascontiguousarray(pts, dtype=f64).reshape(-1, 3)
        self.tri = np.ascontiguousarray(tri, dtype=f32).reshape(-1, 9)
        self.own = np.full(len(self.pts), -1) if own is None else np.asarray(own, dtype=np.int64)
        self.polys = [t.reshape(3, 3) for t in self.tri] if polys is None else polys
        self.marks = marks
        nc, npt = len(self.centers), len(self.pts)
        assert nc <= 64 and npt <= 400 and len(self.tri) <= 600
        self.ci = np.repeat(np.arange(nc, dtype=np.uint32), npt)
        self.pi = np.tile(np.arange(npt, dtype=np.uint32), nc)
        self.cams = cameras_for(self.centers, self.pts)
        self.o, self.d, self.tfar = rays(self.centers[self.ci], self.pts[self.pi])
        self.slots = slots_of(self.tri)
        self.mag = ray_lengths(self.centers[self.ci], self.pts[self.pi])

    @functools.cached_property
    def verdict(self):
        return judge(self.o, self.d, self.tfar, self.slots, own=self.own[self.pi])

    @functools.cached_property
    def closed(self):
        """the mesh's own answer (its vertices as given; the kernels see v0 + (float)(v1 - v0), an ulp away at most)"""
        return closed_exact(self.o, self.d, self.tfar, self.polys)

    def slot_polys(self):
        """the triangles the kernels see, v0, v0 + e1, v0 + e2, exactly (float64 holds the sums)"""
        s = self.slots.astype(f64)
        return [np.stack([r[0:3], r[0:3] + r[3:6], r[0:3] + r[6:9]]) for r in s]


def _r32(a):
    return np.asarray(a, dtype=f64).astype(f32).astype(f64)


_BOX_FACES = ((0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7), (4, 5, 6, 7), (0, 3, 2, 1))


def box_mesh(lo, hi):
    """12 outward triangles (two per face) and the 6 face quads of an axis-aligned box"""
    (x0, y0, z0), (x1, y1, z1) = _r32(lo), _r32(hi)
    c = np.array([(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1), (x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)])
    tri, quads = [], []
    for q in _BOX_FACES:
        tri.append(np.concatenate([c[q[0]], c[q[1]], c[q[2]]]))
        tri.append(np.concatenate([c[q[0]], c[q[2]], c[q[3]]]))
        quads.append(c[list(q)])
    return np.array(tri), quads


def sample_on(tri, which, rng, inset=0.05):
    """one float64 point inside each triangle of `which` (barycentric, `inset` away from every edge)"""
    t = np.asarray(tri, dtype=f32).astype(f64).reshape(-1, 9)[which]
    a, b = rng.uniform(0, 1, len(t)), rng.uniform(0, 1, len(t))
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    a, b = inset + (1 - 3 * inset) * a, inset + (1 - 3 * inset) * b
    return t[:, 0:3] + a[:, None] * (t[:, 3:6] - t[:, 0:3]) + b[:, None] * (t[:, 6:9] - t[:, 0:3])


def _normals(tri):
    t = np.asarray(tri, dtype=f32).astype(f64).reshape(-1, 9)
    n = np.cross(t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _sphere(rng, n, min_axis=0.0):
    out = []
    while len(out) < n:
        v = rng.normal(0, 1, 3)
        v /= np.linalg.norm(v)
        if np.abs(v).min() >= min_axis:
            out.append(v)
    return np.array(out)


# ---- surface -------------------------------------------------------------------------------------------------------
def surface_case(n_boxes, seed):
    rng = np.random.default_rng(seed)
    tri, polys = [], []
    for b in range(n_boxes):
        lo = np.array([3.0 * b - 1.5 * (n_boxes - 1) - 1.0, -1.0 - 0.25 * b, -1.0 + 0.125 * b])
        t, q = box_mesh(lo, lo + np.array([2.0, 2.0 + 0.5 * b, 2.0]))
        tri.append(t); polys += q
    tri = np.concatenate(tri).astype(f32)
    per = 10 if n_boxes == 1 else 2
    own = np.repeat(np.arange(len(tri)), per)
    pts = sample_on(tri, own, rng)
    k = len(tri) * per // 4                                                 # a quarter again, lifted off their faces: clear rays
    t64 = tri.astype(f64).reshape(-1, 3, 3)
    mid = t64.reshape(n_boxes, 36, 3).mean(axis=1)
    nrm = _normals(tri)
    nrm *= np.sign(np.einsum("ij,ij->i", nrm, t64.mean(axis=1) - np.repeat(mid, 12, axis=0)))[:, None]      # outward
    pick = rng.permutation(len(pts))[:k]
    pts = np.concatenate([pts, pts[pick] + 0.3 * nrm[own[pick]]])
    own = np.concatenate([own, np.full(k, -1)])
    n_cam = 24
    radius = np.abs(tri.astype(f64)).max() * np.sqrt(3.0)
    dist = np.geomspace(1.0, 40.0, n_cam)                                  # |dir| brackets 8, 16 and 32
    centers = _sphere(rng, n_cam, 0.1) * (radius + dist)[:, None]
    c = Case("surface-%d" % len(tri), centers, pts, tri, own, polys)
    on = (own >= 0)[c.pi]
    nrm = nrm[np.maximum(own, 0)]
    c.marks["far_face"] = on & (np.einsum("ij,ij->i", nrm[c.pi], c.centers[c.ci] - c.pts[c.pi]) < 0)
    return c


# ---- slivers -------------------------------------------------------------------------------------------------------
def sliver_case(n_tri, seed):
    rng = np.random.default_rng(seed)
    half = n_tri // 2
    tri = []
    for fan, n in enumerate((half, n_tri - half)):
        aspect = np.geomspace(50.0, 5000.0, n)
        ang = np.concatenate([[0.0], np.cumsum(1.0 / aspect)]) + 0.3
        L = 10.0
        rim = np.stack([L * np.cos(ang), L * np.sin(ang), np.zeros(n + 1)], axis=1)
        apex = np.zeros(3)
        if fan == 1:                                                       # the second fan: tilted by 1e-3 rad about x, beside the first
            t = 1e-3
            rot = np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]])
            rim, apex = rim @ rot.T + [0.0, -12.0, 0.5], np.array([0.0, -12.0, 0.5])
        for k in range(n):
            tri.append(np.concatenate([apex, rim[k], rim[k + 1]]))
    tri = np.array(tri).astype(f32)
    n_on = min(160, max(40, 2 * n_tri))
    own = rng.integers(0, n_tri, n_on)
    on = sample_on(tri, own, rng, inset=0.15)
    nrm = _normals(tri)[own]
    k = n_on // 4
    pts = np.concatenate([on, on[:k] + 0.5 * nrm[:k], on[k:2 * k] - 0.5 * nrm[k:2 * k]])      # on, above (clear), below (hidden)
    own = np.concatenate([own, np.full(2 * k, -1)])
    n_cam = 12
    v = _sphere(rng, n_cam, 0.15)
    v[:, 2] = np.abs(v[:, 2]) + 0.5
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    centers = np.array([5.0, -5.0, 0.0]) + v * rng.uniform(20.0, 60.0, n_cam)[:, None]     # further away than the mesh is large
    return Case("slivers-%d" % n_tri, centers, pts, tri, own)


# ---- seams ---------------------------------------------------------------------------------------------------------
def _quad(x0, y0, x1, y1, z):
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    return [np.array(a + b + c, dtype=f64), np.array(a + c + d, dtype=f64)], np.array([a, b, c, d], dtype=f64)


def _hexfan(cx, cy, r):
    ctr = _r32([cx, cy, 0.0])
    rim = _r32([[cx + r * np.cos(np.pi / 3 * k + 0.2), cy + r * np.sin(np.pi / 3 * k + 0.2), 0.0] for k in range(6)])
    return [np.concatenate([ctr, rim[k], rim[(k + 1) % 6]]) for k in range(6)], rim, ctr


SEAM_ULPS = (0, 1, -1, 10, -10, 100, -100)


def seam_case(n_tri, seed):
    """front wall in z = 0 (split quads, 6-fans), a back wall in z = -1 that carries the points; targets on the shared
    edges and vertices, double-rounded (float64, then float32), and SEAM_ULPS float32 ulps beside them in the plane"""
    rng = np.random.default_rng(seed)
    O = 4.0                                                                 # the wall's corner: 100 ulps of a coordinate >= 4 is 5e-5 of a cell
    tri, polys, seams = [], [], []                                         # seams: (target, unit direction of the seam)
    if n_tri == 2:
        grid, fans, back = (1, 1), [], 0
    elif n_tri == 12:
        grid, fans, back = (1, 1), [(3.0, 0.5, 0.7)], 2
    else:
        grid, fans, back = (6, 6), [(8.0, 1.0, 0.8), (8.0, 3.0, 0.9), (8.0, 5.0, 0.7)], 3
    gx, gy = grid
    for i in range(gx):
        for j in range(gy):
            t, _ = _quad(O + i, O + j, O + i + 1.0, O + j + 1.0, 0.0)
            tri += t
            for s in rng.uniform(0.1, 0.9, 2)[: 2 if gx == 1 else int((i, j) in ((1, 4), (3, 2), (5, 0)))]:
                seams.append((np.array([O + i + s, O + j + s, 0.0]), np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)))     # the diagonal
    polys.append(np.array([(O, O, 0), (O + gx, O, 0), (O + gx, O + gy, 0), (O, O + gy, 0)], dtype=f64))
    if gx > 1:
        for i, j in ((2, 3), (4, 1)):                               # inner vertices, and edges between cells
            seams.append((np.array([O + i, O + j, 0.0]), np.array([2.0, -1.0, 0.0]) / np.sqrt(5.0)))     # beside it: off every edge through it
            seams.append((np.array([O + i + rng.uniform(0.2, 0.8), O + j, 0.0]), np.array([1.0, 0.0, 0.0])))
            seams.append((np.array([O + i, O + j + rng.uniform(0.2, 0.8), 0.0]), np.array([0.0, 1.0, 0.0])))
    for cx, cy, r in fans:
        t, rim, ctr = _hexfan(O + cx, O + cy, r)
        tri += t
        polys.append(rim)
        seams.append((ctr, np.array([1.0, 0.0, 0.0])))                      # the fan's vertex
        for k in (0, 3):
            e = rim[k] - ctr
            seams.append((ctr + rng.uniform(0.2, 0.8) * e, e / np.linalg.norm(e)))          # on a spoke
    for b in range(back):
        w = 24.0 / back
        t, q = _quad(O - 8.0 + w * b, O - 9.0, O - 8.0 + w * (b + 1), O + 15.0, -1.0)
        tri += t
        polys.append(q)
    tri = np.array(tri).astype(f32)
    assert len(tri) == n_tri, (len(tri), n_tri)
    mid = np.array([O + gx / 2.0 + (2.0 if fans else 0.0), O + gy / 2.0, 0.0])
    near = mid + np.column_stack([rng.uniform(-2, 2, 2), rng.uniform(-2, 2, 2), rng.uniform(2.0, 5.0, 2)])
    far = mid + np.column_stack([rng.uniform(-3, 3, 4), rng.uniform(-3, 3, 4), np.geomspace(17.0, 40.0, 4)])
    pts, ulps, cam_of = [], [], []
    for tgt, e in seams:
        tgt = _r32(tgt)                                                     # second rounding
        perp = np.array([-e[1], e[0], 0.0])
        step = float(np.spacing(f32(max(abs(tgt[0]), abs(tgt[1]), 0.5))))
        for k in SEAM_ULPS:
            aim = tgt + k * step * perp
            for j, c in enumerate(near):
                xy = aim[:2] + (aim[:2] - c[:2]) / c[2]                     # through `aim`, ending 1 behind the wall
                pts.append([xy[0], xy[1], -1.0]); ulps.append(abs(k)); cam_of.append(j)
    n_aimed = len(pts)
    loose = np.column_stack([O + rng.uniform(0.1, gx - 0.1, 30), O + rng.uniform(0.1, gy - 0.1, 30), np.full(30, 0.5)])
    outside = np.column_stack([O + rng.uniform(-6, -1.5, 20), O + rng.uniform(-6, 12, 20), np.full(20, -1.0)])   # beside the front wall
    pts = np.concatenate([np.array(pts), loose, outside])
    own = np.full(len(pts), -1)
    if back:
        first = n_tri - 2 * back
        for p in np.nonzero(pts[:, 2] == -1.0)[0]:
            for b in range(back):
                w = 24.0 / back
                x0 = O - 8.0 + w * b
                if x0 <= pts[p, 0] <= x0 + w and O - 9.0 <= pts[p, 1] <= O + 15.0:
                    own[p] = first + 2 * b + (0 if (pts[p, 1] - O + 9.0) / 24.0 <= (pts[p, 0] - x0) / w else 1)
    assert len(pts) <= 400, len(pts)
    c = Case("seams-%d" % n_tri, np.concatenate([near, far]), pts, tri, own, polys)
    aimed = np.full(len(c.ci), np.nan)
    for p in range(n_aimed):
        aimed[cam_of[p] * len(pts) + p] = ulps[p]
    c.marks["aimed"] = aimed
    return c


# ---- shielded scenes: grazing, far, switch ---------------------------------------------------------------------------
def shielded_case(name, n_tri, seed, scale=1.0, cam_dist=(17.0, 60.0), shift=0.0, n_cam=16, n_hidden=180, n_clear=100,
                  n_seen=8, specials=False, keep_tri=None):
    """boxes and loose triangles between two big one-triangle walls (z = 0 and z = -5 scale): from the cameras above,
    every point on them is decidedly hidden by the upper wall, and still meets its own triangle at th ~ tfar.  Points
    lifted above the upper wall are decidedly clear; a few points ON the upper wall are seen (open).  With
    specials=True, six more cameras BELOW the lower wall look at triangles there: grazing rays, rays with zero
    direction components, origins on a face of the hierarchy's boxes."""
    rng = np.random.default_rng(seed)
    s = scale
    wall = lambda z: np.array([-40 * s, -30 * s, z, 40 * s, -30 * s, z, 0.0, 50 * s, z])
    tri = [wall(0.0), wall(-5 * s)]
    n_box = (n_tri - 2 - (12 if specials else 3)) // 12
    for b in range(n_box):
        lo = np.array([rng.uniform(-6, 4), rng.uniform(-6, 4), rng.uniform(-4.2, -2.5)]) * s
        tri += list(box_mesh(lo, lo + rng.uniform(0.8, 2.0, 3) * s)[0])
    n_special = 10 if specials else 0
    while len(tri) < n_tri - n_special:
        a = np.array([rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(-4.5, -0.5)]) * s
        tri.append(np.concatenate([a, a + rng.normal(0, 1.2, 3) * s * [1, 1, 0.2], a + rng.normal(0, 1.2, 3) * s * [1, 1, 0.2]]))
    v = _sphere(rng, n_cam, 0.2)
    v[:, 2] = np.abs(v[:, 2]) + 1.0
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    centers = list(v * rng.uniform(cam_dist[0], cam_dist[1], n_cam)[:, None])
    sp_pts, sp_own = [], []
    if specials:
        below = -5 * s
        gcams = [np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), below - rng.uniform(22, 30)]) for _ in range(4)]
        for i, alpha in enumerate(np.geomspace(1e-7, 1e-3, n_special)):        # a triangle at angle alpha to the ray that ends on it
            c = gcams[i % 4]
            p = np.array([rng.uniform(-4, 4), rng.uniform(-4, 4), below - rng.uniform(1.0, 3.0)])
            r = (p - c) / np.linalg.norm(p - c)
            side = np.cross(r, [0.3, 0.5, 0.8]); side /= np.linalg.norm(side)
            up = np.cross(side, r)
            along = np.cos(alpha) * r + np.sin(alpha) * up                     # in the triangle's plane
            t = np.concatenate([p - 1.5 * along - 0.8 * side, p + 1.5 * along - 0.6 * side, p + 0.2 * along + 1.1 * side])
            tri.append(t)
            for q in (p, p + 0.3 * along + 0.1 * side, p - 0.4 * along + 0.2 * side):
                sp_pts.append(q); sp_own.append(len(tri) - 1)
        centers += gcams
    tri = np.array(tri) + shift
    tri = tri.astype(f32)
    assert len(tri) == n_tri, (len(tri), n_tri)
    centers = np.array(centers) + shift
    cand = np.arange(2, (keep_tri or n_tri) - n_special)
    own_h = rng.choice(cand, n_hidden)
    hidden = sample_on(tri, own_h, rng, inset=0.1)
    t0 = tri[0].astype(f64)
    lift = lambda n, h0, h1: np.column_stack([rng.uniform(-5, 5, n) * s + shift, rng.uniform(-5, 5, n) * s + shift,
                                              t0[2] + rng.uniform(h0, h1, n) * s])
    clear = lift(n_clear, 0.5, 2.0)
    seen = lift(n_seen, 0.0, 0.0)
    pts = [hidden, clear, seen]
    own = [own_h, np.full(n_clear, -1), np.zeros(n_seen, dtype=np.int64)]
    if specials:
        sp_pts = np.array(sp_pts) + shift
        zc = np.array([0.0, 0.0, float(tri[1, 2]) - 25.0])                      # zero components: p.x == c.x; -0.0 - +0.0 = -0.0
        zp = np.array([[0.0, 1.5, zc[2] + 20], [-0.0, -2.0, zc[2] + 21], [1.0, 0.0, zc[2] + 20], [2.5, -0.0, zc[2] + 22],
                       [0.0, 0.0, zc[2] + 20], [-0.0, -0.0, zc[2] + 21], [0.0, -0.0, zc[2] + 22], [-0.0, 0.0, zc[2] + 23],
                       [0.0, 3.0, zc[2] + 30], [-0.0, 0.7, zc[2] + 35], [0.6, -0.0, zc[2] + 40], [0.0, 0.0, zc[2] + 40]])
        lo = tri.reshape(-1, 3).min(axis=0)
        margin = f32(np.abs(tri).max()) * f32(4.8e-7) + f32(1e-30)             # bvh_build's box margin
        face = (lo - margin).astype(f32)                                        # a face of a root child's box
        fc = np.array([float(face[0]), -2.0, float(tri[1, 2]) - 24.0])
        fp = np.array([[fc[0], rng.uniform(-4, 4), fc[2] + rng.uniform(15, 30)] for _ in range(6)]
                      + [[rng.uniform(-4, 4), rng.uniform(-4, 4), fc[2] + 20.0] for _ in range(2)])
        centers = np.concatenate([centers, [zc, fc]])
        pts += [sp_pts, zp, fp]
        own += [np.array(sp_own), np.full(len(zp) + len(fp), -1)]
    return Case(name, centers, np.concatenate(pts), tri[:keep_tri], np.concatenate(own))


# ---- tiles ---------------------------------------------------------------------------------------------------------
def tile_case(n_tri, pos, n_rays, seed, lanes=False):
    """one camera, n_rays points (ray = lane): a soup off to the side that no ray meets, a wall triangle at index `pos`,
    and (n_tri > 1) one triangle behind the wall that carries a fifth of the points.  Even lanes end behind the wall,
    odd lanes in front of it.  lanes=True: two walls, the first triangle hiding the odd lanes and the last one the even
    lanes, so half a block has stopped testing in the first tile and still stages every later one."""
    rng = np.random.default_rng(seed)
    a = np.column_stack([rng.uniform(60, 90, n_tri), rng.uniform(-10, 10, n_tri), rng.uniform(-10, 10, n_tri)])
    tri = np.concatenate([a, a + rng.normal(0, 1, (n_tri, 3)), a + rng.normal(0, 1, (n_tri, 3))], axis=1)
    center = np.array([[0.4, -0.3, 30.0]])
    lane = np.arange(n_rays)
    x, y = rng.uniform(-4, 4, n_rays), rng.uniform(-4, 4, n_rays)
    own = np.full(n_rays, -1)
    if lanes:
        tri[0] = [-30, -30, 0, -0.5, -30, 0, -0.5, 40, 0]                      # x < -0.5
        tri[n_tri - 1] = [0.5, -30, 0, 30, -30, 0, 0.5, 40, 0]                 # x > 0.5
        x = np.where(lane % 2 == 1, -np.abs(x) - 1.5, np.abs(x) * 0.5 + 1.5)
        y = y * 0.5 - 4.0
        z = np.full(n_rays, -3.0)
    else:
        tri[pos] = [-40, -30, 0, 40, -30, 0, 0, 50, 0]
        z = np.where(lane % 2 == 0, -3.0, 5.0)
        if n_tri > 1:
            back = 1 if pos != 1 else 2
            tri[back] = [-9, -9, -3, 9, -9, -3, 0, 12, -3]
            on = lane % 10 == 0
            own[on] = back
            x[on], y[on] = x[on] * 0.5, y[on] * 0.5 - 2.0
    pts = np.column_stack([x, y, z])
    return Case("tiles-%d@%d/%d%s" % (n_tri, pos, n_rays, "L" if lanes else ""), center, pts, tri, own)


# ==================================================================================================================
# the families
# ==================================================================================================================
FAMILIES = ("surface", "slivers", "seams", "grazing", "far", "tiles", "switch")
OPEN_CAP = {"grazing": 0.05, "far": 0.05, "tiles": 0.05, "switch": 0.05}


@functools.lru_cache(maxsize=None)
def family(name):
    if name == "surface":
        return [surface_case(1, 11), surface_case(6, 12)]
    if name == "slivers":
        return [sliver_case(n, 20 + n) for n in (8, 64, 200)]
    if name == "seams":
        return [seam_case(n, 30 + n) for n in (2, 12, 96)]
    if name == "grazing":
        return [shielded_case("grazing-70", 70, 41, n_cam=12, n_hidden=220, n_clear=110, specials=True)]
    if name == "far":
        return [shielded_case("far-70", 70, 51, scale=1e-2, cam_dist=(450.0, 550.0)),
                shielded_case("far-70+1e5", 70, 52, scale=8.0, cam_dist=(450.0, 550.0), shift=1e5)]
    if name == "tiles":
        T = K_OCC_TILE
        cases, k = [], 0
        for n_tri in (1, T - 1, T, T + 1, 2 * T, 2 * T + 1):
            for pos in sorted({p for p in (0, T - 1, T, n_tri - 1) if p < n_tri}):
                cases.append(tile_case(n_tri, pos, (K_BLOCK - 1, K_BLOCK, K_BLOCK + 1)[k % 3], 60 + k))
                k += 1
        for n_tri in (T + 1, 2 * T, 2 * T + 1):
            cases.append(tile_case(n_tri, 0, (K_BLOCK + 1, K_BLOCK - 1, K_BLOCK)[k % 3], 60 + k, lanes=True))
            k += 1
        return cases
    if name == "switch":
        return [shielded_case("switch-%d" % n, K_BVH_MIN + 1, 70, n_cam=16, n_hidden=170, n_clear=110, keep_tri=n) for n in
                (K_BVH_MIN - 1, K_BVH_MIN, K_BVH_MIN + 1)]             # the same scene, its last triangles left out
    raise KeyError(name)


def shares(cases):
    """the family's counts over its cases: rays, decided occluded / clear, open, self-hits, thin pairs, contradictions"""
    tot = {"rays": 0, "occluded": 0, "clear": 0, "open": 0, "self_hit": 0, "thin": 0, "contradicted": 0}
    for c in cases:
        v = c.verdict
        tot["rays"] += len(c.ci)
        for k in ("occluded", "clear", "open", "self_hit"):
            tot[k] += int(v[k].sum())
        tot["thin"] += v["thin"]
        tot["contradicted"] += v["contradicted"]
    return tot
