"""The noise / statistics reference and its bound (tests/_noiseref.py), made trustworthy on the CPU before they judge a
kernel (tests/test_gpu_noise_reference.py):
  * the f64 restatement of the kernels lies inside C E of the long-double reference on every problem the GPU tests use;
  * so does the CPU oracle -- a correct implementation with libm in place of the lean transcendentals passes;
  * each one-line mutation of the restatement lands OUTSIDE the bound somewhere (and the test says where);
  * the axis-aligned grid of tests/test_gpu_parity.py cannot see some of them."""
import functools

import numpy as np
import pytest

import _noiseref as N
import oracle as O
from _problems import (NOISE_COUNT_PAIRS, PLANAR_Y, STATS_TOTALS, grid_cameras_points, grid_problem, noise_base as base,
                       noise_cases as all_cases, stats_points)


@functools.lru_cache(maxsize=None)
def case(label):
    _, kind, variant, n_cam, n_pts, over = next(c for c in all_cases() if c[0] == label)
    P = base(variant)
    cams, pts = P["cams15"][:n_cam], P["pts"][:n_pts]
    rec = N.stats_record(cams, pts)
    prm = dict(N.PASSES[kind], **over)
    return kind, cams, pts, rec, prm, N.evaluate(kind, cams, pts, rec, prm)


def _oracle(kind, cams, pts, prm):
    if kind == "drift":
        return O.add_drift(cams, pts, prm["strength"], prm["angle_strength"], prm["std"], np.array(prm["dir"]), prm["seed"])
    if kind == "drift_normalized":
        return O.add_drift_normalized(cams, pts, prm["strength"], prm["angle_strength"], prm["std"], prm["seed"])
    if kind == "noise":
        return O.add_noise(cams, pts, np.zeros((0, 2)), prm["translation_std"], prm["rotation_std"], prm["point_std"], 0.0,
                           prm["seed"])[:2]
    return O.add_sin_noise(cams, pts, prm["dir"], prm["noise_dir"], prm["strength"], prm["frequency"])


def test_philox_and_the_long_double_draws_are_the_oracles():
    ent = np.array([0, 1, 77, 2 ** 32 + 5, 2 ** 40 + 123456789], dtype=np.uint64)
    for seed, stream, slot in ((42, 1, 0), (2 ** 40 + 99, 3, 2), (7, 4, 1)):
        words = np.stack(N.philox4x32_10(ent, ent >> np.uint64(32), slot, stream, seed, seed >> 32), axis=1)
        z = N.normal_pairs(seed, stream, ent, (slot,))[:, 0]
        for i, e in enumerate(ent):
            want = O.philox4x32_10([int(e) & 0xFFFFFFFF, int(e) >> 32, slot, stream], [seed & 0xFFFFFFFF, seed >> 32])
            assert np.array_equal(words[i].astype(np.uint32), want)
            zo = O.normal_pair(seed, stream, int(e), slot)
            rad = float(np.hypot(*z[i].astype(np.float64)))
            assert np.all(np.abs(zo - z[i]).astype(np.float64) <= N.U * (N.DRAW_REL * np.abs(zo) + N.DRAW_ABS * rad))


def test_inputs_are_what_the_cases_claim():
    P = base("planar")
    cen, _ = N.device_centers(P["cams15"])
    assert len(cen) == 300 and np.all(cen[:, 1] == PLANAR_Y) and np.all(P["pts"][:, 1] == PLANAR_Y)      # bit for bit
    assert N.stats_record(P["cams15"], P["pts"])[13] == 0.0
    far = base("far")
    rec = N.stats_record(far["cams15"][:65], far["pts"])
    assert np.all(rec[12:15] > 390.0)
    ref = N.drift(far["cams15"][:65], far["pts"], rec[15:18], 1e-5, 0.3, 0.2, (0.3, -0.5, 0.8), *N.drift_draws(42, 65, 700))
    assert 200.0 < float(np.abs(ref[2]["angle"]).max()) < 1000.0               # drift angles of hundreds of radians
    _, cams, pts, rec, prm, _ = case("noise/300x700")
    ang = 4.0 * N.noise_draws(prm["seed"], 300, 0)[0][:, 1, 1]
    assert float(np.abs(ang).max()) > np.pi                                    # rotation noise beyond pi at rotation_std = 4
    for c in base(None)["cams15"], far["cams15"], P["cams15"]:
        assert np.all(c[:, 13:15] != 0.0) and len(np.unique(c[:, 12:15].view(np.uint64))) == c[:, 12:15].size


def test_the_origin_is_an_entity_at_distance_zero_with_no_angle_and_no_displacement():
    for n_cam, n_pts in ((65, 700), (65, 0), (1, 0), (0, 1)):
        P = base(None)
        cams, pts = P["cams15"][:n_cam], P["pts"][:n_pts]
        rec = N.stats_record(cams, pts)
        i = int(rec[18])
        prm = N.PASSES["drift"]
        zc, zp = N.drift_draws(prm["seed"], n_cam, n_pts)
        ref = N.drift(cams, pts, rec[15:18], prm["strength"], prm["angle_strength"], prm["std"], prm["dir"], zc, zp)
        out = N.k_add_drift(cams, pts, rec[15:18], prm["strength"], prm["angle_strength"], prm["std"], prm["dir"], zc, zp)
        if i >= n_cam:                                       # a point: its bits are the origin's
            j = i - n_cam
            assert ref[2]["d_pt"][j] == 0 and np.array_equal(ref[1][j].astype(np.float64), pts[j])
            assert np.array_equal(out[2][j], pts[j])
            if n_pts > 4:
                assert j == 4 and np.array_equal(pts[0], pts[4])         # the tie went to the later entity
        else:                                                # a camera: the origin is the centre as the kernels compute it
            cen, e_cen = N.device_centers(cams)
            assert np.array_equal(rec[15:18], cen[i])
            d_max = float(e_cen[i].sum())                    # the reference's centre is within e_cen of these bits: |.|_2 <= |.|_1
            assert float(ref[2]["d_cam"][i]) <= d_max        # 0 up to the rounding of that centre ...
            big = abs(prm["strength"]) * (1 + prm["std"] * float(np.abs(zc[i]).max()))          # ... and so are the angle and the move
            assert abs(float(ref[2]["angle"][i])) <= abs(prm["angle_strength"]) / abs(prm["strength"]) * big * d_max ** np.float64(1.2) * (1 + N.U)
            assert float(np.abs(ref[2]["move"][i]).max()) <= float(np.abs(prm["dir"]).max()) * big * d_max * d_max * (1 + N.U)
            assert np.array_equal(out[0][i, 0:9], N.k_add_drift(cams, pts, rec[15:18], 0.0, 0.0, 0.0, prm["dir"], zc, zp)[0][i, 0:9])


@pytest.mark.parametrize("label", [c[0] for c in all_cases()])
def test_restatement_and_oracle_lie_inside_the_bound(label):
    kind, cams, pts, rec, prm, r = case(label)
    msgs = [N.report(r["c"], r["ref_c"], r["Ec"], label + " restatement cameras"),
            N.report(r["p"], r["ref_p"], r["Ep"], label + " restatement points")]
    assert np.array_equal(r["c"][:, 12:15].view(np.uint64), cams[:, 12:15].view(np.uint64))
    # the oracle takes its statistics itself: hand the reference the same inputs (its std / |std|; origin and dimensions are
    # selections and agree exactly)
    orec = rec.copy()
    orec[3:6] = O.std(cams, pts)
    orec[19] = np.sqrt((orec[3] * orec[3] + orec[4] * orec[4]) + orec[5] * orec[5])
    o, idx = O.drift_origin(cams, pts)
    assert idx == int(rec[18]) and np.array_equal(o, rec[15:18])
    assert np.array_equal(O.dimensions(cams, pts), rec[12:15])
    ro = N.evaluate(kind, cams, pts, orec, prm, oracle=True)            # the bound of libm's draws (DRAW_ABS): the oracle's only
    oc, op = _oracle(kind, cams, pts, prm)
    msgs += [N.report(oc, ro["ref_c"], ro["Ec"], label + " oracle cameras"), N.report(op, ro["ref_p"], ro["Ep"], label + " oracle points")]
    assert not any(msgs), "\n".join(m for m in msgs if m)


def test_zero_std_and_zero_strength_are_what_they_should_be():
    kind, cams, pts, rec, prm, r = case("std=0/drift")
    zc, zp = N.drift_draws(prm["seed"], len(cams), len(pts))
    zero = N.drift(cams, pts, rec[15:18], prm["strength"], prm["angle_strength"], 0.2, prm["dir"], 0 * zc, 0 * zp)
    assert np.array_equal(zero[0], r["ref_c"]) and np.array_equal(zero[1], r["ref_p"])        # the factor is exactly 1
    kind, cams, pts, rec, prm, r = case("zero-strength/drift")
    assert np.array_equal(r["p"], pts) and np.array_equal(r["ref_p"].astype(np.float64), pts)
    ident = N.transform(cams, np.broadcast_to(np.eye(3, dtype=N.LD), (len(cams), 3, 3)), np.zeros(3, dtype=N.LD))
    assert not N.report(r["c"], ident, r["Ec"], "transform by the identity")


# ---- statistics ----------------------------------------------------------------------------------------------------
def _stat_cases():
    """every total of STATS_TOTALS (points only), every count pair, the variants"""
    out = [("points/%d" % n, None, 0, n) for n in STATS_TOTALS]
    out += [("pairs/%dx%d" % (c, p), None, c, p) for (c, p) in NOISE_COUNT_PAIRS]
    return out + [("offset/points/5000", "offset", 0, 5000), ("offset/points/%d" % (512 * 256 + 1), "offset", 0, 512 * 256 + 1),
                  ("offset/300x700", "offset", 300, 700), ("planar/300x700", "planar", 300, 700)]


def _stat_entities(label, variant, n_cam, n_pts):
    if "points/" in label:                                   # the totals: points only, the tie spanning the table
        return np.zeros((0, 15)), stats_points(n_pts, 21, variant)
    P = base(variant)
    return P["cams15"][:n_cam], P["pts"][:n_pts]


@pytest.mark.parametrize("label,variant,n_cam,n_pts", _stat_cases())
def test_statistics_restatement_and_oracle_lie_inside_the_bound(label, variant, n_cam, n_pts):
    cams, pts = _stat_entities(label, variant, n_cam, n_pts)
    cen, e_cen = N.device_centers(cams)
    ent = np.concatenate([cen, pts])
    ref = N.statistics(cams, pts, centers_=cen)
    got, depth = N.k_stats(ent)
    E = N.stats_bound(ent, depth)
    assert not N.report(got, ref, E, label + " restatement")
    if depth <= N.device_depth(len(ent)):                    # a tree no deeper than the device's: inside the bound the GPU test uses
        assert not N.report(got, ref, N.stats_bound(ent, N.device_depth(len(ent))), label + " restatement at the device's depth")
    bad, _ = N.k_stats(ent, mutations=("chan_nb",))
    if len(ent) > N.STAT_BATCH:                              # at least one merge: the wrong weight leaves the bound of either depth
        assert np.any(N.outside(bad[3:6], ref[3:6], N.stats_bound(ent, max(depth, N.device_depth(len(ent))))[3:6])), label
    exact, want = N.exact_slots(ref)
    assert np.array_equal(got[exact], want)
    orc = np.zeros(20)
    orc[0:3], orc[3:6] = O.mean(cams, pts), O.std(cams, pts)
    orc[6:9], orc[9:12] = O.extent(cams, pts)
    orc[12:15] = O.dimensions(cams, pts)
    o, idx = O.drift_origin(cams, pts)
    orc[15:18], orc[18] = o, idx
    orc[19] = ref[19].astype(np.float64)                                 # the oracle has no |std| entry of its own
    assert not N.report(orc, ref, N.stats_bound(ent, len(ent)), label + " oracle (a sequential fold: depth n)")
    assert np.array_equal(orc[exact], want)
    # the long-double centres agree with the computed ones to their bound: the record of -R^T t is the same record
    if n_cam:
        assert not N.report(N.statistics(cams, pts).astype(np.float64)[:6], ref[:6], N.stats_bound(ent, depth, e_ent=e_cen)[:6], label)


def test_a_single_pass_variance_fails_on_the_offset_cloud():
    """sum x^2 / n - mean^2 in f64 -- the formula the (count, mean, M2) triples replace -- is far outside the bound on the
    cloud whose offset dwarfs its spread: the case that separates the two"""
    pts = stats_points(5000, 21, "offset")
    ref = N.statistics(np.zeros((0, 15)), pts)
    E = N.stats_bound(pts, N.device_depth(len(pts)))
    naive = np.sqrt(np.abs((pts * pts).mean(axis=0) - pts.mean(axis=0) ** 2))
    assert np.all(N.outside(naive, ref[3:6], E[3:6]))
    assert np.all(N.resolved(E[3:6], ref[3:6].astype(np.float64)))       # ... and the tolerance is below the spread it judges


# ---- mutations -------------------------------------------------------------------------------------------------------
def _outside(dev, ref, E):
    if not np.asarray(dev).size:
        return False
    return bool(np.any(N.outside(dev, ref, E)))


def _seen_by(mutation, labels):
    """the first case of `labels` on which the mutated restatement leaves the bound, or None"""
    for label in labels:
        kind, cams, pts, rec, prm, r = case(label)
        with np.errstate(all="ignore"):
            m = N.evaluate(kind, cams, pts, rec, prm, mutations=(mutation,), reference=False)
        if _outside(m["c"], r["ref_c"], r["Ec"]) or _outside(m["p"], r["ref_p"], r["Ep"]):
            return label
    return None


def _stats_seen_by(mutation, ents):
    for label, ent in ents:
        ref = N.statistics(np.zeros((0, 15)), ent)
        got, depth = N.k_stats(ent, mutations=(mutation,))
        if _outside(got, ref, N.stats_bound(ent, depth)):
            return label
    return None


WHERE = {"dR_R": "drift/300x700", "center_R": "drift/300x700", "rot_y": "drift/300x700", "pow_1": "drift/300x700",
         "dist_1": "drift/300x700", "draws_swapped": "drift/300x700", "no_bal_std": "noise/300x700", "no_eps": "planar/sin",
         "noise_dir_raw": "sin/300x700", "chan_nb": "stats 300x700", "origin_tie_earlier": "stats 300x700"}


@pytest.mark.parametrize("mutation", N.MUTATIONS)
def test_each_mutation_lands_outside_the_bound(mutation):
    P = base(None)
    ents = [("stats 300x700", np.concatenate([N.device_centers(P["cams15"])[0], P["pts"]]))]
    if mutation in ("chan_nb", "origin_tie_earlier"):
        seen = _stats_seen_by(mutation, ents)
    else:
        seen = _seen_by(mutation, ["drift/300x700", "noise/300x700", "sin/300x700", "planar/sin"])
    assert seen == WHERE[mutation], "%s (%s): seen by %r" % (mutation, N.MUTATION_TEXT[mutation], seen)


GRID_BLIND = frozenset({"no_eps", "noise_dir_raw"})


def test_the_axis_aligned_grid_cannot_see_some_mutations():
    """The one problem the noise kernels were compared on before (tests/test_gpu_parity.py: _grid_problem(), with the
    parameters of its tests) under the same mutations and THIS file's bound: the mutations in GRID_BLIND stay inside the
    bound on every entry there -- the general-position problems above see every one of them."""
    G = grid_problem()
    cams, pts = G["cams15"], G["pts"]
    rec = N.stats_record(cams, pts)
    runs = [("drift", dict(strength=1e-3, angle_strength=2e-3, std=0.2, dir=(0.3, -0.5, 0.8), seed=42)),
            ("drift_normalized", dict(strength=0.1, angle_strength=0.1, std=0.1, seed=7)),
            ("noise", dict(translation_std=0.1, rotation_std=0.1, point_std=0.1, seed=99)),
            ("sin", dict(dir=(1.0, 1.0, 0.0), noise_dir=(0.0, 1.0, 0.0), strength=1.0, frequency=2.0))]
    refs = [(k, p, N.evaluate(k, cams, pts, rec, p)) for k, p in runs]
    ent = np.concatenate([N.device_centers(cams)[0], pts])
    blind = set()
    for mutation in N.MUTATIONS:
        if mutation in ("chan_nb", "origin_tie_earlier"):
            seen = _stats_seen_by(mutation, [("grid", ent)]) is not None
        else:
            seen = False
            for k, p, r in refs:
                with np.errstate(all="ignore"):
                    m = N.evaluate(k, cams, pts, rec, p, mutations=(mutation,), reference=False)
                seen = seen or _outside(m["c"], r["ref_c"], r["Ec"]) or _outside(m["p"], r["ref_p"], r["Ep"])
        if not seen:
            blind.add(mutation)
    assert blind == GRID_BLIND and blind, sorted(blind)


def test_the_float_files_per_entry_tolerance_is_never_looser_than_the_global_bound_it_replaced():
    """tests/test_gpu_f32.py judged every entry by 4e-6 ... 2e-5 times the largest entry of the array; it now uses the
    u = 2^-24 bound per entry.  On its state and its parameters that tolerance is at most the old bound on EVERY entry."""
    cams, pts = grid_cameras_points(3, cpb=10, ppb=20, L=5.0)
    c32, p32 = cams.astype(np.float32).astype(np.float64), pts.astype(np.float32).astype(np.float64)
    rec = N.stats_record(c32, p32)
    for kind, prm, old_c, old_p in N.F32_FILE_RUNS:
        r = N.evaluate(kind, c32, p32, rec, prm, u=N.U32)
        bc, bp = N.f32_old_bounds(r, old_c, old_p)
        assert bc is None or np.all(N.tolerance(r["Ec"][:, :12], r["ref_c"][:, :12]) <= bc), kind
        assert np.all(N.tolerance(r["Ep"], r["ref_p"]) <= bp), kind


def test_the_float_sine_pass_cannot_resolve_the_planar_cloud():
    """y / 1e-8 makes angles of ~1e8 rad, known in float to tens of radians: the bound is the cap there, and says so"""
    P = base("planar")
    rec = N.stats_record(P["cams15"], P["pts"])
    prm = N.PASSES["sin"]
    r32 = N.evaluate("sin", P["cams15"].astype(np.float32).astype(np.float64), P["pts"].astype(np.float32).astype(np.float64),
                     rec, prm, u=N.U32, reference=False)
    r64 = N.evaluate("sin", P["cams15"], P["pts"], rec, prm, reference=False)
    assert not np.any(N.resolved(r32["Ep"].max(axis=1), prm["strength"]))
    assert np.all(N.resolved(r64["Ep"].max(axis=1), prm["strength"]))
