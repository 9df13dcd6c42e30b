"""The noise kernels (k_add_drift, k_add_noise_entities, k_add_sin_noise, double and float) and the statistics pass
(k_stats_pass1) against the extended-precision reference of tests/_noiseref.py, entry by entry, inside the running
bound of the kernels' own order of operations: |dev - ref| <= C E + |ref| 2^-60 + FLOOR.  tests/test_noiseref.py shows on
the CPU that a correct implementation passes this bound on the same inputs and that one-line mistakes do not.

The kernels take the statistics record as an argument: the tests hand them the reference's record (rounded to f64), so
each kernel is judged apart from the statistics pass, and the standard normals are the reference's own Box-Muller of
the same Philox words, so the arithmetic is judged apart from the draw (which has its own test below).

Every table is allocated with GUARD rows of a sentinel bit pattern behind its end and passed as the leading slice:
a store past the end (wave_rows_store writes whole waves of 64 records) shows up as a changed sentinel.  The cameras'
intrinsics (columns 12..14, distinct bit patterns) and the points' fourth lane must come back bit for bit.

Worst |dev - ref| / E per kernel and scalar type are printed (run with -s) and recorded in DESIGN.md."""
import ctypes as C

import numpy as np
import pytest

import _noiseref as N
from _problems import (NOISE_COUNT_PAIRS, NOISE_KINDS as KINDS, STATS_TOTALS, noise_base as base, noise_edge_cases as edge_cases,
                       stats_points)

pytestmark = pytest.mark.gpu

GUARD = 64
SENT64 = 0x7FF8DEAD0000BEEF            # a quiet NaN with a payload no kernel produces
SENT32 = 0x7FC0BEEF


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build()
    import torch
    import city2ba_amd
    from city2ba_amd import _lib as L
    from city2ba_amd import device as D
    assert city2ba_amd.device_count() > 0, "no HIP device: the gpu tests must run on the GPU box"
    dev = torch.device("cuda", 0)
    return dict(torch=torch, c2b=city2ba_amd, D=D, L=L, dev=dev, ws=D.workspace(0, dev))


def _guarded(env, rows, f32):
    """rows [n, w] on the device with GUARD sentinel rows behind them: (whole allocation as integers, the leading slice)"""
    torch = env["torch"]
    n, w = rows.shape
    it, ft, sent = (torch.int32, torch.float32, SENT32) if f32 else (torch.int64, torch.float64, SENT64)
    whole = torch.full((n + GUARD, w), sent, dtype=it, device=env["dev"])
    view = whole.view(ft)[:n]
    if n:
        view.copy_(torch.from_numpy(np.array(rows, dtype=np.float32 if f32 else np.float64, order="C")).to(env["dev"]))
    assert view.is_contiguous() and view.shape == (n, w)
    return whole, view, sent


def _pts4(pts):
    """[n, 4]: the fourth lane holds a different value in every row"""
    return np.concatenate([pts, 1000.0 + np.arange(len(pts), dtype=np.float64)[:, None]], axis=1)


def _launch(env, kind, c, p, st, prm, f32):
    D, L = env["D"], env["L"]
    if kind == "drift":
        if f32:
            D.add_drift_f32(c, p, st, prm["strength"], prm["angle_strength"], prm["std"], prm["dir"], prm["seed"])
        else:
            D.add_drift_sharded(c, 0, p, st, prm["strength"], prm["angle_strength"], prm["std"], prm["seed"], direction=prm["dir"])
    elif kind == "drift_normalized":
        if f32:
            D.add_drift_normalized_f32(c, p, st, prm["strength"], prm["angle_strength"], prm["std"], prm["seed"])
        elif prm.get("sharded_entry"):
            D.add_drift_sharded(c, 0, p, st, prm["strength"], prm["angle_strength"], prm["std"], prm["seed"])
        else:
            D.add_drift_normalized(c, p, st, prm["strength"], prm["angle_strength"], prm["std"], prm["seed"])
    elif kind == "noise":
        f = D.add_noise_entities_f32 if f32 else D.add_noise_entities
        f(c, p, st, prm["translation_std"], prm["rotation_std"], prm["point_std"], prm["seed"])
    elif f32:
        D.add_sin_noise_f32(c, p, st, prm["dir"], prm["noise_dir"], prm["strength"], prm["frequency"])
    else:
        # the f64 sine pass has no Level-0 wrapper in device.py: the C entry c2b.noise.add_sin_noise launches, with this record
        d, nd = [float(x) for x in prm["dir"]], [float(x) for x in prm["noise_dir"]]
        L.check(L.lib().c2b_add_sin_noise(C.c_void_p(c.data_ptr()), c.shape[0], C.c_void_p(p.data_ptr()), p.shape[0],
                                          C.c_void_p(st.data_ptr()), d[0], d[1], d[2], nd[0], nd[1], nd[2],
                                          float(prm["strength"]), float(prm["frequency"]),
                                          C.c_void_p(env["torch"].cuda.current_stream().cuda_stream)))


def run_pass(env, kind, cams, pts, prm, f32, label):
    """One kernel over (cams, pts) behind guard rows with the reference's record.  Returns (messages, worst |err| / E,
    device cameras, device points, the evaluation)."""
    torch = env["torch"]
    if f32:
        cams, pts = cams.astype(np.float32).astype(np.float64), pts.astype(np.float32).astype(np.float64)
    rec = N.stats_record(cams, pts)
    r = N.evaluate(kind, cams, pts, rec, prm, u=N.U32 if f32 else N.U)
    p4 = _pts4(pts)
    cw, c, sent = _guarded(env, cams, f32)
    pw, p, _ = _guarded(env, p4, f32)
    st = torch.from_numpy(rec).to(env["dev"])
    _launch(env, kind, c, p, st, prm, f32)
    torch.cuda.synchronize()
    gc = c.cpu().numpy()
    gp = p.cpu().numpy()
    n_cam, n_pts = len(cams), len(pts)
    msgs = []
    if not bool((cw[n_cam:] == sent).all().item()):
        msgs.append("%s: sentinel rows behind the camera table changed" % label)
    if not bool((pw[n_pts:] == sent).all().item()):
        msgs.append("%s: sentinel rows behind the point table changed" % label)
    it = np.uint32 if f32 else np.uint64
    ft = np.float32 if f32 else np.float64
    if not np.array_equal(gc[:, 12:15].view(it), cams[:, 12:15].astype(ft).view(it)):
        msgs.append("%s: intrinsics (columns 12..14) are not the input's bits" % label)
    if not np.array_equal(gp[:, 3].view(it), p4[:, 3].astype(ft).view(it)):
        msgs.append("%s: the points' fourth lane is not the input's bits" % label)
    gc64, gp64 = gc.astype(np.float64), gp[:, :3].astype(np.float64)
    msgs.append(N.report(gc64[:, :12], r["ref_c"][:, :12], r["Ec"][:, :12], label + " cameras"))
    msgs.append(N.report(gp64, r["ref_p"], r["Ep"], label + " points"))
    with np.errstate(invalid="ignore"):
        worst = max(N.ratio(gc64[:, :12], r["ref_c"][:, :12], r["Ec"][:, :12]) if n_cam else 0.0,
                    N.ratio(gp64, r["ref_p"], r["Ep"]) if n_pts else 0.0)
    return [m for m in msgs if m], worst, gc64, gp64, r


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_kernel_at_every_count_pair(env, kind, f32):
    """n_cam in {0, 1, 63, 64, 65, 255, 256, 257, 300} x n_pts in {0, 1, 5, 700}: whole waves of cameras leave through LDS
    (15 values), the wave that straddles the camera / point boundary per lane (12 values)"""
    P = base(None)
    msgs, worst = [], 0.0
    for n_cam, n_pts in NOISE_COUNT_PAIRS:
        if kind == "drift_normalized" and n_cam + n_pts == 1:
            continue                                          # std() = 0 has no direction: NaN in the reference as well (CPU file)
        m, w, _, _, _ = run_pass(env, kind, P["cams15"][:n_cam], P["pts"][:n_pts], N.PASSES[kind], f32, "%s/%dx%d" % (kind, n_cam, n_pts))
        msgs += m
        worst = max(worst, w if np.isfinite(w) else np.inf)
    print("\nWORST |dev - ref| / E  %s %s: %.3f" % (kind, "f32" if f32 else "f64", worst))
    assert not msgs, "\n".join(msgs)


def test_a_single_entity_has_no_normalized_drift_direction(env):
    """std() of one entity is 0: dir = 0 / 0 in the reference (src/noise.rs:53) and here -- NaN in, nothing else touched"""
    P = base(None)
    for n_cam, n_pts in ((0, 1), (1, 0)):
        m, _, gc, gp, _ = run_pass(env, "drift_normalized", P["cams15"][:n_cam], P["pts"][:n_pts], N.PASSES["drift_normalized"], False, "single")
        assert not m, "\n".join(m)
        assert np.all(np.isnan(gp)) and np.all(np.isnan(gc[:, 9:12]))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("label", [c[0] for c in edge_cases()])
def test_edge_variants(env, label, f32):
    """planar (a zero dimension: 1e-8 substituted), far (drift angles of hundreds of radians), rotation noise beyond pi,
    std = 0 (the factor is exactly 1: the reference with z = 0, tests/test_noiseref.py), zero strength (points bit-equal,
    cameras = transform by the identity).  The float sine pass cannot resolve the planar cloud -- angles of ~1e8 rad known
    to tens of radians: its bound is the cap of 2 on a sine (tests/test_noiseref.py asserts that), so planar/sin-f32 checks
    the store path, the intrinsics and finiteness only; the double pass is resolved and judged."""
    _, kind, variant, n_cam, n_pts, over = next(c for c in edge_cases() if c[0] == label)
    P = base(variant)
    prm = dict(N.PASSES[kind], **over)
    m, worst, gc, gp, r = run_pass(env, kind, P["cams15"][:n_cam], P["pts"][:n_pts], prm, f32, label)
    print("\nWORST |dev - ref| / E  %s %s: %.3f" % (label, "f32" if f32 else "f64", worst))
    assert not m, "\n".join(m)
    assert np.all(np.isfinite(gc)) and np.all(np.isfinite(gp))
    if label == "zero-strength/drift":
        pts = P["pts"][:n_pts]
        assert np.array_equal(gp, pts.astype(np.float32).astype(np.float64) if f32 else pts)


def test_the_drift_origin_does_not_move(env):
    """the entity that is the origin has distance exactly 0 (pow_lean's library fallback): a point keeps its bits; a
    camera is judged by run_pass like every entry (the reference's own distance is 0 up to the rounding of its centre)"""
    P = base(None)
    for n_cam, n_pts in ((65, 700), (65, 0)):
        cams, pts = P["cams15"][:n_cam], P["pts"][:n_pts]
        m, _, gc, gp, _ = run_pass(env, "drift", cams, pts, N.PASSES["drift"], False, "origin")
        assert not m, "\n".join(m)
        i = int(N.stats_record(cams, pts)[18])
        assert (i >= n_cam) == bool(n_pts)
        if i >= n_cam:
            assert np.array_equal(gp[i - n_cam], pts[i - n_cam])


def test_normalized_drift_through_the_sharded_entry(env):
    P = base(None)
    prm = dict(N.PASSES["drift_normalized"], sharded_entry=True)
    m, _, _, _, _ = run_pass(env, "drift_normalized", P["cams15"][:257], P["pts"][:5], prm, False, "sharded entry")
    assert not m, "\n".join(m)


def test_planar_cloud_through_the_problem_level_sine_pass(env):
    """c2b.noise.add_sin_noise on a resident problem: the device's own statistics see the zero dimension"""
    c2b = env["c2b"]
    P = base("planar")
    cams, pts = P["cams15"][:65], P["pts"]
    prm = N.PASSES["sin"]
    rec = N.stats_record(cams, pts)
    assert rec[13] == 0.0
    r = N.evaluate("sin", cams, pts, rec, prm)
    ba = c2b.BAProblem.from_visibility(cams, pts, np.zeros(len(cams) + 1, dtype=np.uint64), [], np.zeros((0, 2)))
    assert np.array_equal(ba.dimensions(), rec[12:15])
    ba = c2b.noise.add_sin_noise(ba, prm["dir"], prm["noise_dir"], prm["strength"], prm["frequency"])
    msgs = [N.report(ba.cameras()[:, :12], r["ref_c"][:, :12], r["Ec"][:, :12], "cameras"), N.report(ba.points(), r["ref_p"], r["Ep"], "points")]
    assert not any(msgs), "\n".join(msgs)
    assert np.array_equal(ba.cameras()[:, 12:15].view(np.uint64), cams[:, 12:15].view(np.uint64))


# ---- statistics ------------------------------------------------------------------------------------------------------
def _stats_check(env, cams, pts, label, centers_route=False):
    torch, D, dev, ws = env["torch"], env["D"], env["dev"], env["ws"]
    n_cam = len(cams)
    pts4 = D.points_pad(torch.from_numpy(np.array(pts, order="C")).to(dev))
    cen4 = D.centers_table(n_cam, dev)
    if n_cam:
        blk = D.cameras_prepare_state(torch.from_numpy(np.array(cams, order="C")).to(dev), centers=cen4)
    else:
        blk = torch.zeros((0, 32), dtype=torch.float64, device=dev)
    a = D.stats(blk, pts4, ws).cpu().numpy()
    b = D.stats(blk, pts4, ws).cpu().numpy()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), label + ": a second call on the same workspace differs (ticket re-arming)"
    if centers_route:
        c = D.stats(blk, pts4, ws, centers=cen4).cpu().numpy()
        assert np.array_equal(a.view(np.uint64), c.view(np.uint64)), label + ": centers= and the record route differ"
    cen = cen4.cpu().numpy()[:, :3]
    e_cen = None
    if n_cam:
        want_cen, e_cen = N.device_centers(cams)
        msg = N.report(cen, N.centers(cams), e_cen, label + " centres")
        assert not msg, msg
    ent = np.concatenate([cen, pts])
    ref = N.statistics(cams, pts, centers_=cen)               # over the centres the device holds: selections stay exact
    E = N.stats_bound(ent, N.device_depth(len(ent)))
    exact, want = N.exact_slots(ref)
    assert np.array_equal(a[exact], want), "%s: min / max / dimensions / origin / index\n%r\n%r" % (label, a[exact], want)
    msg = N.report(a, ref, E, label)
    assert not msg, msg
    soft = [0, 1, 2, 3, 4, 5, 19]
    return N.ratio(a[soft], ref[soft], E[soft])


@pytest.mark.parametrize("n", STATS_TOTALS)
def test_statistics_at_the_count_edges_of_the_reduction(env, n):
    """points only: one lane, a batch tail, a wave, a workgroup, four workgroups, the grid cap of 512 workgroups, each +- 1,
    and four entities per thread at the cap plus three; the first and the last point tie for the origin"""
    pts = stats_points(n, 21)
    w = _stats_check(env, np.zeros((0, 15)), pts, "points/%d" % n)
    print("\nWORST |dev - ref| / E  statistics %d points: %.4f" % (n, w))


@pytest.mark.parametrize("n", [5000, 512 * 256 + 1])
def test_statistics_of_a_cloud_whose_offset_dwarfs_its_spread(env, n):
    """1e6 away, 1e-3 wide: a single-pass variance is garbage here (tests/test_noiseref.py), the (count, mean, M2) triples are not"""
    pts = stats_points(n, 21, "offset")
    w = _stats_check(env, np.zeros((0, 15)), pts, "offset/%d" % n)
    print("\nWORST |dev - ref| / E  statistics offset %d points: %.4f" % (n, w))


@pytest.mark.parametrize("n_cam,n_pts", NOISE_COUNT_PAIRS)
def test_statistics_at_every_count_pair_and_through_the_centres_table(env, n_cam, n_pts):
    """every (n_cam, n_pts) pair of the noise tests: the record route and `centers=` bit for bit, a second call bit for bit"""
    P = base(None)
    _stats_check(env, P["cams15"][:n_cam], P["pts"][:n_pts], "%dx%d" % (n_cam, n_pts), centers_route=True)


def test_statistics_of_the_planar_and_offset_problems_with_cameras(env):
    for variant in ("planar", "offset"):
        P = base(variant)
        _stats_check(env, P["cams15"], P["pts"], variant, centers_route=True)


# ---- the entity draw ---------------------------------------------------------------------------------------------------
N_DRAWS = 1 << 20


def _draw_check(got, seed, stream, which, label):
    """got = the device's standard normal per entity; the reference: Box-Muller of the same Philox words in long double.
    Tolerance: 2 ulps of 2 (the two additions that carry the draw out of the kernel: 1 + z, then 1 + that, each half an ulp
    of a number below 8) plus C u |z| (1 + |ln u1|) for the lean logarithm / sine / cosine."""
    ent = np.arange(N_DRAWS)
    z = N.normal_pairs(seed, stream, ent, (0,))[:, 0, which]
    u1, _ = N.uniforms(seed, stream, ent, 0)
    assert float(np.abs(z).max()) < 6.0                       # so that 2 + z stays below 8
    zt = N.U * np.abs(z).astype(np.float64) * (1.0 + np.abs(np.log(u1)).astype(np.float64))
    tol = 2 * 2.0 ** -51 + N.C * zt
    err = np.abs(got.astype(N.LD) - z).astype(np.float64)
    worst = float(np.max((err - 2 * 2.0 ** -51) / zt))
    print("\nWORST (|z_dev - z_ref| - 2 ulp(2)) / (u |z| (1 + |ln u1|))  %s: %.3f of C = %g; max |err| %.3e" % (label, worst, N.C, err.max()))
    bad = np.flatnonzero(err > tol)
    assert bad.size == 0, "%s: %d draws outside the tolerance, first entity %d: |err| %.3e tol %.3e" % (label, bad.size, bad[0], err[bad[0]], tol[bad[0]])


def test_the_point_streams_draw_against_box_muller_in_long_double(env):
    """(1, 0, 0) rows, origin (0, 0, 0), dir (1, 0, 0), strength = std = 1, no angle: p.x = 1 + (1 + z0), every other
    factor being exactly 1"""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    pts4 = torch.zeros((N_DRAWS, 4), dtype=torch.float64, device=dev)
    pts4[:, 0] = 1.0
    cam15 = torch.zeros((0, 15), dtype=torch.float64, device=dev)
    st = torch.zeros(20, dtype=torch.float64, device=dev)
    D.add_drift_sharded(cam15, 0, pts4, st, 1.0, 0.0, 1.0, 4242, direction=(1.0, 0.0, 0.0))
    got = pts4.cpu().numpy()
    assert np.all(got[:, 1:] == 0.0)
    _draw_check(got[:, 0] - 2.0, 4242, N.STREAM_DRIFT_PT, 0, "point stream z0")


def test_the_camera_streams_draw_against_box_muller_in_long_double(env):
    """identity cameras at centre (1, 0, 0): t = (-1, 0, 0); the translation draw is z1: t'.x = -(1 + (1 + z1)), and the
    rotation stays the identity bit for bit (angle strength 0)"""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    row = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, -1, 0, 0, 1.0, 0.0, 0.0])
    cam15 = torch.from_numpy(row).to(dev).repeat(N_DRAWS, 1).contiguous()
    pts4 = torch.zeros((0, 4), dtype=torch.float64, device=dev)
    st = torch.zeros(20, dtype=torch.float64, device=dev)
    D.add_drift_sharded(cam15, 0, pts4, st, 1.0, 0.0, 1.0, 777, direction=(1.0, 0.0, 0.0))
    got = cam15.cpu().numpy()
    assert np.array_equal(got[:, 0:9], np.broadcast_to(row[0:9], (N_DRAWS, 9))) and np.all(got[:, 10:12] == 0.0)
    assert np.array_equal(got[:, 12:15], np.broadcast_to(row[12:15], (N_DRAWS, 3)))
    _draw_check(-got[:, 9] - 2.0, 777, N.STREAM_DRIFT_CAM, 1, "camera stream z1")
