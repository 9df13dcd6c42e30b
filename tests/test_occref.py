"""The occlusion reference (tests/_occref.py) held against itself, the conditions its ray families must meet, and -- without
a GPU -- everything about the occlusion step that is host arithmetic: the C oracle's orc_occlusion_filter against the float32
restatement, and the real c2b_bvh_build hierarchy walked in numpy: for every (ray, slot) pair the restatement accepts,
every box on the slot's path from the root must pass the slab test, so that the hierarchy cannot prune a hit the
all-triangles loop finds."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import _occref as R
import oracle as O

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_hip()
    O.build()
    from city2ba_amd import _lib as L
    return L


def test_rays_are_formed_as_the_kernels_form_them():
    c = np.array([[0.1, 0.2, 0.3], [1e5 + 0.123, -7.0, 2.0], [0.0, 0.0, 0.0]])
    p = np.array([[1.1, 2.2, 3.3], [1e5 + 3.0, 20.0, 2.0], [-0.0, 0.0, 40.0]])
    o, d, tfar = R.rays(c, p)
    assert o.dtype == d.dtype == tfar.dtype == f32
    for i in range(3):
        e = p[i] - c[i]
        mag = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        inv = 1.0 / mag
        assert np.array_equal(o[i], c[i].astype(f32))
        assert np.array_equal(d[i].view(np.uint32), np.array([e[0] * inv, e[1] * inv, e[2] * inv]).astype(f32).view(np.uint32))
        assert tfar[i] == f32(mag) - f32(1e-6)
    assert np.signbit(d[2, 0]) and d[2, 0] == 0 and not np.signbit(d[2, 1])          # -0.0 - +0.0 = -0.0 survives
    assert np.array_equal(R.slots_of(np.arange(9, dtype=f32)[None] ** 2)[0],
                          np.array([0, 1, 4, 9 - 0, 16 - 1, 25 - 4, 36 - 0, 49 - 1, 64 - 4], dtype=f32))


def test_exact_values_and_outcomes_against_fractions():
    """long double against exact rationals on pairs of every kind: values to 2^-58 of the terms' magnitude, outcomes equal
    (the thin pairs are settled by the Fraction path itself: here the others are)"""
    rng = np.random.default_rng(0)
    n = 0
    for name in ("surface", "slivers", "seams"):
        c = R.family(name)[-1]
        rr = rng.integers(0, len(c.ci), 12)
        x = R.exact(c.o[rr], c.d[rr], c.tfar[rr], c.slots)
        for a, r in enumerate(rr):
            for t in rng.integers(0, len(c.tri), 6):
                F = lambda v: [Fraction(float(q)) for q in v]
                o, d, s = F(c.o[r]), F(c.d[r]), F(c.slots[t])
                cross = lambda p, q: [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]
                dot = lambda p, q: sum(pi * qi for pi, qi in zip(p, q))
                v0, e1, e2 = s[0:3], s[3:6], s[6:9]
                pv = cross(d, e2)
                det = dot(e1, pv)
                assert tuple(x["cmp"][:, a, t]) == R._fraction_signs(c.o[r], c.d[r], c.tfar[r], c.slots[t])
                if det == 0:
                    continue
                tv = [o[k] - v0[k] for k in range(3)]
                qv = cross(tv, e1)
                want = {"u": dot(tv, pv) / det, "w": dot(d, qv) / det, "th": dot(e2, qv) / det}
                mag = {"u": dot([abs(v) for v in tv], [abs(v) for v in pv]), "w": dot([abs(v) for v in d], [abs(v) for v in qv]),
                       "th": dot([abs(v) for v in e2], [abs(v) for v in qv])}
                for k in want:
                    err = abs(Fraction(float(x[k][a, t])) + Fraction(float(x[k][a, t] - R.LD(float(x[k][a, t])))) - want[k])
                    assert err <= Fraction(2) ** -58 * (mag[k] / abs(det) + abs(want[k])) * 64, (name, r, t, k)
                n += 1
    assert n > 150


def test_fraction_path_agrees_with_long_double_where_both_are_decided():
    """exact() with THIN raised so that every pair goes through Fraction gives the outcomes long double gave"""
    c = R.family("seams")[1]
    rr = np.arange(0, len(c.ci), 7)
    a = R.exact(c.o[rr], c.d[rr], c.tfar[rr], c.slots)
    thin = R.THIN
    try:
        R.THIN = 1e300
        b = R.exact(c.o[rr], c.d[rr], c.tfar[rr], c.slots)
    finally:
        R.THIN = thin
    assert b["thin"] == len(rr) * len(c.slots) and a["thin"] < b["thin"]
    assert np.array_equal(a["cmp"], b["cmp"])


def test_thin_pairs_are_settled_exactly():
    """a ray through a quad's diagonal and one in a triangle's plane: long double sees 0 or noise, Fraction decides"""
    tri = np.array([[0, 0, 0, 1, 0, 0, 1, 1, 0], [0, 0, 0, 1, 1, 0, 0, 1, 0]], dtype=f32)
    o, d, tfar = R.rays([[0.5, 0.5, 2.0], [-3.0, 0.25, 0.0]], [[0.5, 0.5, -1.0], [5.0, 0.25, 0.0]])
    x = R.exact(o, d, tfar, R.slots_of(tri))
    assert x["thin"] >= 3
    assert x["hit"][0].all()                                   # on the shared edge: both closed triangles are met
    assert not x["cmp"][0, 1].any()                            # in the plane: det == 0 exactly, no crossing
    assert np.array_equal(R.closed_exact(o, d, tfar, [tri[0].reshape(3, 3), tri[1].reshape(3, 3)]), [True, False])
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=f32)
    assert np.array_equal(R.closed_exact(o, d, tfar, [quad]), [True, False])


def test_vectorised_tests_equal_the_scalar_ones():
    from test_bvh_host import mt_hit, box_hit
    c = R.family("grazing")[0]
    rng = np.random.default_rng(1)
    rr, tt = rng.integers(0, len(c.ci), 300), rng.integers(0, len(c.tri), 300)
    got = R.mt_hit(c.o[rr], c.d[rr], c.tfar[rr], c.slots[tt])
    assert np.array_equal(got, [mt_hit(c.o[r], c.d[r], c.tfar[r], c.slots[t]) for r, t in zip(rr, tt)])
    assert np.array_equal(got, R.hits_f32(c.o, c.d, c.tfar, c.slots)[rr, tt])
    lo = c.tri.reshape(-1, 3, 3).min(axis=1)[tt] - f32(1.5)
    hi = c.tri.reshape(-1, 3, 3).max(axis=1)[tt] + f32(1.5)
    with np.errstate(all="ignore"):
        inv = f32(1.0) / c.d[rr]
        want = [bool(box_hit(lo[k], hi[k], c.o[rr[k]], inv[k], c.tfar[rr[k]])) for k in range(300)]
    assert np.array_equal(R.box_hit(lo, hi, c.o[rr], inv, c.tfar[rr]), want)
    assert 10 < sum(want) < 290


@pytest.mark.parametrize("name", R.FAMILIES)
def test_bound_is_never_contradicted_and_the_two_exact_answers_agree(name):
    """no decided pair is answered differently by the restatement or by exact arithmetic; decided occluded implies
    met in exact arithmetic, decided clear implies not; and closed_exact (planes and polygons, float64 + Fraction)
    gives the union that exact() (Moeller-Trumbore numerators, long double + Fraction) gives triangle by triangle"""
    for c in R.family(name):
        v = c.verdict
        assert v["contradicted"] == 0, c.name
        assert not (v["occluded"] & v["clear"]).any()
        assert np.array_equal(v["f32"][v["occluded"]], np.ones(int(v["occluded"].sum()), bool)), c.name
        assert not v["f32"][v["clear"]].any(), c.name
        assert v["exact"][v["occluded"]].all() and not v["exact"][v["clear"]].any(), c.name
        assert np.array_equal(R.closed_exact(c.o, c.d, c.tfar, c.slot_polys()), v["exact"]), c.name
        # the mesh as given (merged coplanar polygons, unrounded edges) differs from that only where (float)(v1 - v0)
        # rounds, by an ulp of an edge: never on a decided ray
        assert not (c.closed != v["exact"])[~v["open"]].any(), c.name


@pytest.mark.parametrize("name", R.FAMILIES)
def test_caps(name, capsys):
    """conditions on the INPUTS, from the reference alone (DESIGN 3.6 records the shares)"""
    cases = R.family(name)
    s = R.shares(cases)
    with capsys.disabled():
        print("\n%-8s rays %6d  decided occluded %5.1f %%  decided clear %5.1f %%  open %5.1f %%  self-hits %5d  thin pairs %d"
              % (name, s["rays"], 100.0 * s["occluded"] / s["rays"], 100.0 * s["clear"] / s["rays"], 100.0 * s["open"] / s["rays"],
                 s["self_hit"], s["thin"]))
    assert s["occluded"] >= 100 and s["clear"] >= 100
    assert s["self_hit"] >= 200                              # rays that meet their own triangle at th <= tfar: the tfar edge is tested
    if name in R.OPEN_CAP:
        assert s["open"] <= R.OPEN_CAP[name] * s["rays"]
    for c in cases:
        v = c.verdict
        if "far_face" in c.marks:
            ff = c.marks["far_face"]
            assert ff.sum() > 1000 and v["occluded"][ff].all(), c.name
        if "aimed" in c.marks:
            a = c.marks["aimed"]
            assert (a >= 100).sum() >= 8 and not v["open"][a >= 100].any(), c.name
            assert (a < 100).sum() >= 20
        # tfar at the surface: (float)|dir| - 1e-6f.  The subtraction rounds away where half an ulp of |dir| exceeds 1e-6,
        # i.e. from |dir| >= 32 (ulp 3.8e-6); in [8, 32) it lands exactly one ulp below (ulps 9.5e-7 and 1.9e-6).
        m32 = c.mag.astype(f32)
        assert np.array_equal(c.tfar[c.mag >= 32], m32[c.mag >= 32]), c.name
        mid = (c.mag >= 8) & (c.mag < 31.9)
        assert np.array_equal(c.tfar[mid], np.nextafter(m32[mid], f32(0))), c.name
    if name == "surface":
        mag = np.concatenate([c.mag for c in cases])
        for lo, hi in ((1, 8), (8, 16), (16, 32), (32, 80)):                 # |dir| brackets 8, 16 and 32
            assert ((mag >= lo) & (mag < hi)).sum() >= 300
        for c in cases:                                                       # the facades at the mesh's extreme coordinates carry points
            ext = np.abs(c.tri).max()
            on = c.own >= 0
            assert (np.abs(c.pts[on]).max(axis=1) == ext).sum() >= 2
            assert (c.pts[on].min(axis=0) == c.tri.reshape(-1, 3).min(axis=0)).any()
    if name == "grazing":
        c = cases[0]
        with np.errstate(all="ignore"):
            inv = f32(1.0) / c.d
        zero = (c.d == 0).sum(axis=1)
        assert (zero == 1).sum() >= 8 and (zero == 2).sum() >= 4
        assert np.isposinf(inv).any() and np.isneginf(inv).any()
        n = R._normals(c.tri)
        sin = np.abs(np.einsum("rj,tj->rt", c.d.astype(f64), n))
        own = c.own[c.pi]
        graze = sin[np.arange(len(own)), np.maximum(own, 0)][own >= 0]
        assert ((graze > 0) & (graze < 2e-3)).sum() >= 20 and ((graze > 0) & (graze < 1e-5)).sum() >= 5
    if name == "tiles":
        T, B = R.K_OCC_TILE, R.K_BLOCK
        assert {len(c.tri) for c in cases} == {1, T - 1, T, T + 1, 2 * T, 2 * T + 1}
        assert {len(c.ci) for c in cases} == {B - 1, B, B + 1}
        for c in cases:                                                       # the soup decides nothing: only walls are ever met
            h = c.verdict["hits"]
            assert h.sum(axis=0).astype(bool).sum() <= 2 + 1, c.name
    if name == "switch":
        assert [len(c.tri) for c in cases] == [R.K_BVH_MIN - 1, R.K_BVH_MIN, R.K_BVH_MIN + 1]
        assert all(np.array_equal(c.tri[:R.K_BVH_MIN - 1], cases[0].tri) for c in cases)


@pytest.mark.parametrize("name", R.FAMILIES)
def test_oracle_equals_restatement(lib, name):
    for c in R.family(name):
        keep = O.occlusion_filter(c.cams, c.pts, c.ci, c.pi, c.tri)
        assert np.array_equal(O.centers(c.cams), c.centers), c.name          # axis-looking cameras: exact centres
        assert np.array_equal(keep == 0, c.verdict["f32"]), c.name
        assert np.array_equal(R.occluded_numpy(c.centers[c.ci], c.pts[c.pi], c.tri), c.verdict["f32"])


@functools.lru_cache(maxsize=None)
def _hierarchy(name):
    """(accepted pairs, pairs a box on the path would prune, worst tn - tfar in ulps of tfar, the numpy traversal equals the
    all-triangles mask) over the family's cases"""
    pruned = accepted = 0
    worst, same = -np.inf, True
    for c in R.family(name):
        nodes, slots, order, depth = R.bvh_build(c.tri)
        assert np.array_equal(slots[:, :9], c.slots[order])
        p, a, w = R.pruned_hits(c.o, c.d, c.tfar, nodes, slots)
        pruned, accepted, worst = pruned + p, accepted + a, max(worst, w)
        same &= np.array_equal(R.traverse(c.o, c.d, c.tfar, nodes, slots), c.verdict["f32"])
    return accepted, pruned, worst, same


@pytest.mark.parametrize("name", R.FAMILIES)
def test_hierarchy_never_prunes_an_accepted_hit(lib, name, capsys):
    """the real c2b_bvh_build boxes and the device's slab test restated: along the path to every slot the restatement
    accepts, every box passes; and the numpy traversal of the whole hierarchy gives the all-triangles mask.  (With the
    bare `tn <= tfar` the hierarchy had until this test existed, 253 of the `far` family's accepted pairs were pruned
    and 17 of its rays answered differently.)"""
    accepted, pruned, worst, same = _hierarchy(name)
    with capsys.disabled():
        print("\n%-8s accepted (ray, slot) pairs %6d  pruned by a box on the path %d  worst tn - tfar %+.1f ulps of tfar"
              % (name, accepted, pruned, worst))
    assert accepted >= 200 and pruned == 0 and same
    if name == "grazing":
        # origins exactly ON a face of a box of the real hierarchy (the mesh's lowest x less bvh_build's margin), with
        # d.x == 0: (lo - o) * (1 / d) = 0 * inf is NaN in the slab test, which then must not constrain (the traversal above
        # answered these rays as the all-triangles loop does)
        c = R.family(name)[0]
        nodes = R.bvh_build(c.tri)[0]
        with np.errstate(all="ignore"):
            nan = np.isnan((nodes[0][[0, 6]][None, :] - c.o[:, None, 0]) * (f32(1.0) / c.d[:, None, 0])).any(axis=1)
        assert nan.sum() >= 6


def test_slab_slack_is_16_times_the_worst_measured(lib):
    """bvh_box_hit accepts tn <= tfar * 1.00001f: 1e-5 relative is at least 83 ulps of tfar; the worst tn - tfar over the
    accepted pairs of every family must stay 16 times below that"""
    worst = max(_hierarchy(name)[2] for name in R.FAMILIES)
    assert 1e-5 / 2.0 ** -23 > 83
    assert 0 <= worst and 16 * worst <= 83, worst
