"""The camera conversions and the camera table held to a reference of their own (tests/_camref.py): from_vec
(k_cameras_from_bal, k_cameras_prepare<true>), to_vec (k_cameras_to_bal, k_cameras_prepare<false>), the centre field and
the cen4 side table (k_cameras_prepare<*>, k_cameras_centers) -- at every branch of from_rodrigues, cm_quat_from_mat and
to_rodrigues, on matrices that are rotations only to 1e-14 or not at all, and at the camera counts where the wave-private
write-out changes shape, behind canaries.  Two kinds of check:
  sharp     against the arithmetic restated in f64 in the kernel's order: bit for bit where no sin / cos / acos enters,
            within ACOS_ULP ulps of the angle where acos does;
  reference against longdouble forms that do not follow the kernel (exp_so3, log_ld, the residual R c + t), within C E of
            the restatement's running bound.
tests/test_camref.py checks the checker on the CPU."""
import ctypes

import numpy as np
import pytest

import _camref as R
import _jacref as J

pytestmark = pytest.mark.gpu

LD = J.LD
CANARY = np.uint64(0x7FF8DEADBEEF0BAD)                 # a quiet NaN with a payload no kernel produces
TWO60 = 2.0 ** -60


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build()
    import torch
    import city2ba_amd
    from city2ba_amd import _lib as L
    from city2ba_amd import device as D
    assert city2ba_amd.device_count() > 0
    return dict(torch=torch, D=D, L=L, c2b=city2ba_amd, dev=torch.device("cuda", 0))


@pytest.fixture(scope="module")
def fams():
    return R.families()


def _up(env, a):
    return env["torch"].from_numpy(np.array(a, order="C")).to(env["dev"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _to_rowmajor9(Rcm):
    return np.ascontiguousarray(R.rowmajor(Rcm).reshape(-1, 9))


def _labels(label, err, E, what):
    """per label: the worst |err| / E and the worst absolute error"""
    for key in dict.fromkeys(label):
        s = label == key
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err[s] == 0, 0.0, err[s] / np.maximum(E[s], J.FLOOR))
        print("[camera reference]   %s %-14s worst |err|/E = %.3g, worst |err| = %.3g" % (what, key, r.max(), err[s].max()))


# ---- from_vec ----------------------------------------------------------------------------------------------------
def test_from_vec(env, fams):
    D = env["D"]
    f = fams["angles"]
    b, label = f["bal9"], f["label"]
    cam = D.cameras_from_bal(_up(env, b)).cpu().numpy()
    rec = D.camblk_records(D.cameras_prepare_bal(_up(env, b))).cpu().numpy()
    Rv, Er, small = R.from_vec(b)
    assert small.sum() > 50 and (~small).sum() > 50
    # sharp: no sin / cos on the small-angle branch
    assert _same(cam[small, 0:9], Rv[small]), "from_vec: the small-angle branch is not the restated arithmetic bit for bit"
    # reference
    ref = R.colmajor(J.exp_so3(b[:, 0:3]))
    err = np.abs(cam[:, 0:9] - ref).astype(np.float64)
    _labels(label, err, Er, "from_vec |w| =")
    bad = R.outside(cam[:, 0:9], ref, Er)
    assert not bad.any(), "from_vec: %d entries outside C E, first at |w| = %s" % (bad.sum(), label[np.argwhere(bad)[0][0]])
    print("[camera reference] angles/from_vec (k_cameras_from_bal): worst |err|/E = %.3g" % R.ratio(cam[:, 0:9], ref, Er))
    # t and the intrinsics copied; the table's kernel gives the same bits
    assert _same(cam[:, 9:15], b[:, 3:9])
    assert _same(rec[:, 0:9], _to_rowmajor9(cam[:, 0:9])), "k_cameras_prepare<true> and k_cameras_from_bal disagree on R"
    assert _same(rec[:, 9:15], b[:, 3:9])
    # orthonormality, to the size the bound implies: (R + dR)^T (R + dR) - I = R^T dR + dR^T R + dR^T dR
    Rd = R.rowmajor(cam[:, 0:9].astype(LD))
    G = np.abs(np.einsum("nki,nkj->nij", Rd, Rd) - np.eye(3, dtype=LD)).astype(np.float64)
    Ed = R.rowmajor(Er)
    A = np.abs(R.rowmajor(cam[:, 0:9]))
    B = np.einsum("nki,nkj->nij", A, Ed) + np.einsum("nki,nkj->nij", Ed, A) + np.einsum("nki,nkj->nij", Ed, Ed)
    _labels(label, G.reshape(-1, 9), B.reshape(-1, 9), "|R^T R - I| at |w| =")
    assert np.all(G <= J.C * B + J.FLOOR)


# ---- to_vec ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FAMILIES)
def test_to_vec(env, fams, name):
    D = env["D"]
    f = fams[name]
    cam, label = f["cam15"], f["label"]
    got = D.cameras_to_bal(_up(env, cam)).cpu().numpy()
    w = np.ascontiguousarray(got[:, 0:3])
    W, E, masks = R.to_vec(cam, rotation=f["rotation"])
    zero = masks[3]
    # ---- sharp: against the restated arithmetic
    assert np.array_equal((w == 0.0).all(axis=1), zero), "%s: exact zeros are not exactly where the restated 1 - q0^2 < eps" % name
    assert _same(w[zero], W[zero])
    d = np.abs(w - W)
    assert np.all(d <= R.sharp_tolerance(W)), "%s: %d components beyond ACOS_ULP = %g ulps of the restated to_vec (worst %.3g ulps)" % (
        name, int(np.sum(d > R.sharp_tolerance(W))), R.ACOS_ULP, float(np.max(d / np.maximum(np.spacing(np.abs(W)), J.FLOOR))))
    assert _same(got[:, 3:9], cam[:, 9:15])
    nz = ~zero
    ang = np.sqrt((W[nz] * W[nz]).sum(axis=1))
    ulps = (d[nz].max(axis=1) / np.spacing(ang)).max() if nz.any() else 0.0
    print("[camera reference] %s/to_vec: device against the restatement with acos rounded once from longdouble: worst %.3g ulps of the angle"
          % (name, ulps))
    # ---- the same to_vec behind the table's J_l field (k_cameras_prepare<false>)
    rec = D.camblk_records(D.cameras_prepare_state(_up(env, cam))).cpu().numpy()
    assert _same(rec[:, 0:9], _to_rowmajor9(cam[:, 0:9])) and _same(rec[:, 9:15], cam[:, 9:15])
    Jl = J.left_jacobian(*(J.V(w[:, k]) for k in range(3)))
    want, Ej = np.stack([x.v for x in Jl], axis=1), np.stack([x.e for x in Jl], axis=1)
    series = ((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]) < 1e-2
    assert _same(rec[series, 15:24], want[series]), "%s: the table's J_l is not left_jacobian of cameras_to_bal's vector" % name
    refj = J.left_jacobian_ld(w).reshape(-1, 9)
    assert np.all(np.abs(rec[:, 15:24] - refj).astype(np.float64) <= J.tolerance(Ej, refj))
    if not f["rotation"]:
        print("[camera reference] %s/to_vec: no rotations -- sharp check only (%d cameras, %d exact zeros)" % (name, len(cam), zero.sum()))
        return
    # ---- reference: the representative the device must produce
    dl = R.defect(cam[:, 0:9])
    ref_w, other, either = R.log_ld(cam[:, 0:9], dl)
    ref = R.nearest(w, ref_w, other, either)
    err = np.abs(w - ref).astype(np.float64)
    _labels(label, err, E, "to_vec")
    bad = R.outside(w, ref, E)
    assert not bad.any(), "%s/to_vec: %d entries outside C E, first at %s" % (name, bad.sum(), label[np.argwhere(bad)[0][0]])
    # ---- representative-free: exp of what came back is the matrix that went in
    back = R.colmajor(J.exp_so3(w))
    Eb = R.exp_bound(E, dl)
    assert np.all(np.abs(back - cam[:, 0:9].astype(LD)).astype(np.float64) <= J.C * Eb + J.FLOOR), name
    print("[camera reference] %s/to_vec (k_cameras_to_bal): worst |err|/E = %.3g against log, %.3g through exp; %d either-sign cameras"
          % (name, R.ratio(w, ref, E), R.ratio(back, cam[:, 0:9].astype(LD), Eb), either.sum()))


def test_round_trips(env, fams):
    """to_vec(from_vec(w)) against w, within the bound of to_vec fed with from_vec's.  The rotation's principal vector p is w
    below pi and w - 2 pi w / |w| between pi and 3 pi (the 2 pi of this family lies a few 1e-16 to either side of it, by axis).
    p comes back wherever the quaternion's q0 comes out positive: on the trace branch (|p| <= 2 pi / 3) always, on the other
    three -- they make the DOMINANT component of the quaternion positive, whatever that does to q0 -- when the dominant
    component of p's axis is positive.  Otherwise the formula, which is the reference's, returns the representative longer
    than pi, p - 2 pi p / |p|: w - 2 pi w / |w| for a w between 2 pi / 3 and pi, w itself for a w between pi and 4 pi / 3.
    Each camera is held to the ONE representative that log_ld's rule (the sign of the branch's q0, in longdouble on exp(w))
    gives it; only at |w| = np.pi, where that sign is its own rounding, either passes."""
    D = env["D"]
    f = fams["angles"]
    b, label = f["bal9"], f["label"]
    w2 = D.cameras_to_bal(D.cameras_from_bal(_up(env, b))).cpu().numpy()[:, 0:3]
    Rv, Er, _ = R.from_vec(b)
    _, E, _ = R.to_vec(np.column_stack([Rv, b[:, 3:9]]), R_err=Er)
    wl = b[:, 0:3].astype(LD)
    nrm = np.sqrt((wl * wl).sum(axis=1))
    unit = wl / np.where(nrm > 0, nrm, LD(1))[:, None]
    sel = nrm < 3 * R.PI_LD
    assert set(label[~sel]) == {"100"}
    same, turned = wl, wl - 2 * R.PI_LD * unit
    rule, _, either = R.log_ld(R.colmajor(J.exp_so3(b[:, 0:3])), Er.max(axis=1))
    assert set(label[either & sel]) == {"pi"}                       # |w| = np.pi: the sign of q0 is its own rounding
    d_same, d_turned = (np.abs(rule - x).max(axis=1).astype(np.float64) for x in (same, turned))
    assert np.all(np.minimum(d_same, d_turned)[sel] <= 2.0 ** -50)   # the rule's pick is one of the two
    takes_turned = d_turned < d_same
    want = R.nearest(w2, np.where(takes_turned[:, None], turned, same), np.where(takes_turned[:, None], same, turned), either)
    below = sel & ~either & (nrm < R.PI_LD)
    assert not np.any(takes_turned[below & (nrm < 2.0)]), "w itself must return while the trace is positive"
    print("[camera reference] angles/round trip: %d of %d cameras with 2 pi / 3 < |w| < pi return as w - 2 pi w / |w|, %d of %d with pi < |w| < 3 pi"
          % (takes_turned[below & (nrm > 2.0)].sum(), (below & (nrm > 2.0)).sum(), takes_turned[sel & ~either & (nrm > R.PI_LD)].sum(),
             (sel & ~either & (nrm > R.PI_LD)).sum()))
    err = np.abs(w2 - want).astype(np.float64)
    _labels(label[sel], err[sel], E[sel], "to_vec(from_vec(w)) |w| =")
    bad = R.outside(w2[sel], want[sel], E[sel])
    assert not bad.any(), "round trip: %d entries outside C E, first at |w| = %s" % (bad.sum(), label[sel][np.argwhere(bad)[0][0]])
    print("[camera reference] angles/round trip: worst |err|/E = %.3g" % R.ratio(w2[sel], want[sel], E[sel]))


# ---- centres -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FAMILIES)
def test_centres(env, fams, name):
    D, dev = env["D"], env["dev"]
    f = fams[name]
    b = R.bal9_of(f)                                            # the family's own 9-vectors, or the restated to_vec of its matrices
    forms = [("state", f["cam15"], D.cameras_prepare_state, f["cam15"]),
             ("bal", b, D.cameras_prepare_bal, D.cameras_from_bal(_up(env, b)).cpu().numpy())]
    for form, inp, prepare, cam in forms:
        cen = D.centers_table(len(inp), dev)
        cen.fill_(float("nan"))
        rec = D.camblk_records(prepare(_up(env, inp), centers=cen)).cpu().numpy()
        cen = cen.cpu().numpy()
        assert _same(cen[:, 0:3], rec[:, 24:27]), "%s/%s: cen4 is not the record's centre field" % (name, form)
        assert np.all(_bits(cen[:, 3]) == 0) and np.all(_bits(rec[:, 27:32]) == 0)
        c, Ec = R.center(cam)
        assert _same(cen[:, 0:3], c), "%s/%s: the centre is not cm_center's arithmetic bit for bit" % (name, form)
        res, scale = R.center_residual(cam, cen[:, 0:3])
        res, B = np.abs(res).astype(np.float64), R.center_bound(cam, Ec)
        assert np.all(res <= J.C * B + scale.astype(np.float64) * TWO60 + J.FLOOR), "%s/%s" % (name, form)
        with np.errstate(divide="ignore", invalid="ignore"):
            print("[camera reference] %s/centre (%s): worst |R c + t| / E = %.3g" % (name, form, np.where(res == 0, 0.0, res / np.maximum(B, J.FLOOR)).max()))


def test_centres_refreshed_from_the_state(env, fams):
    """k_cameras_centers against the centres k_cameras_prepare<false> writes, on cameras that are rotations only to 1e-14.  The
    kernel is reachable at Level 1 only: c2b_problem_stats derives the centre table with it whenever the camera table is stale
    and the cameras are in state mode (compute_stats: !blk_valid && !bal_valid) -- after a drift, and after any upload through
    from_visibility, which prepares no table.  The other side must therefore be made to read a table that k_cameras_prepare
    wrote: at Level 0 (cameras_prepare_state and device.stats with its centers=), where no other kernel can have written it, and
    at Level 1 after _camera_centers(), whose c2b_problem_centers goes through ensure_camblk and leaves blk_valid set, so that
    the statistics that follow take the table's branch.  One camera alone makes the statistics the centre itself."""
    torch, D, c2b, dev = env["torch"], env["D"], env["c2b"], env["dev"]
    from city2ba_amd import noise as N
    cam = fams["drifted"]["cam15"]
    pts = np.random.default_rng(5).uniform(-30, 30, size=(50, 3))
    empty = lambda n: (np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2)))
    ba = c2b.BAProblem.from_visibility(cam, pts, *empty(len(cam)))
    before = ba._stats()                                              # k_cameras_centers (a fresh upload in state mode)
    N.add_drift_normalized(ba, 1e-3, 1e-4, 1e-2, seed=3)
    moved = ba._stats()                                               # k_cameras_centers (the drift left the table stale)
    assert not _same(moved, before)
    moved_cam, moved_pts = ba.cameras(), ba.points()
    # Level 0: the table and the centres of k_cameras_prepare<false>, the same statistics pass over them
    cen = D.centers_table(len(cam), dev)
    cen.fill_(float("nan"))
    table = D.cameras_prepare_state(_up(env, moved_cam), centers=cen)
    level0 = D.stats(table, D.points_pad(_up(env, moved_pts)), D.workspace(0, dev), centers=cen).cpu().numpy()
    assert _same(moved, level0), "the statistics over k_cameras_centers' table are not those over k_cameras_prepare's"
    centres = cen.cpu().numpy()[:, 0:3]
    assert _same(centres, R.center(moved_cam)[0])
    # Level 1: a fresh upload made to prepare its table first
    fresh = c2b.BAProblem.from_visibility(moved_cam, moved_pts, *empty(len(cam)))
    assert _same(fresh._camera_centers(), centres)                    # ensure_camblk: k_cameras_prepare<false>, blk_valid set
    assert _same(fresh._stats(), moved)                               # ... so these read the table's centres
    # camera by camera: a problem of one camera and no point has that camera's centre as its minimum, maximum and origin
    want, _ = R.center(cam)
    for i in range(0, len(cam), 8):
        s = c2b.BAProblem.from_visibility(cam[i:i + 1], np.zeros((0, 3)), *empty(1))._stats()      # k_cameras_centers
        assert _same(s[6:9], want[i]) and _same(s[9:12], want[i]), "camera %d: k_cameras_centers is not cm_center's arithmetic" % i
        assert _same(s[15:18], want[i]) and int(s[18]) == 0           # ... and is the entity nearest the origin


# ---- camera counts at which the write-out changes shape ----------------------------------------------------------
def _canary(env, shape):
    return env["torch"].from_numpy(np.full(shape, CANARY, dtype=np.uint64).view(np.float64)).to(env["dev"])


def _run_four(env, cam, bal, n, rows, table_doubles):
    """the four kernels on the first n cameras into canary-filled buffers of `rows` rows / `table_doubles` doubles; everything as
    uint64: dict(from_bal [rows, 15], to_bal [rows, 9], and per prepare form records [n, 32], flat, cen [rows, 4])"""
    torch, D, L = env["torch"], env["D"], env["L"]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    o15, o9 = _canary(env, (rows, 15)), _canary(env, (rows, 9))
    L.check(L.lib().c2b_cameras_from_bal(ptr(bal), n, ptr(o15), stream))
    L.check(L.lib().c2b_cameras_to_bal(ptr(cam), n, ptr(o9), stream))
    out["from_bal"], out["to_bal"] = o15, o9
    for form, prepare, inp in (("state", D.cameras_prepare_state, cam), ("bal", D.cameras_prepare_bal, bal)):
        flat, cen = _canary(env, (table_doubles,)), _canary(env, (rows, 4))
        table = prepare(inp[:n], out=D.CameraTable(n, env["dev"], flat), centers=cen[:n])
        out[form] = (table.records(), flat, cen)
    torch.cuda.synchronize()
    u = lambda t: _bits(t.cpu().numpy())
    return {k: tuple(u(x) for x in v) if isinstance(v, tuple) else u(v) for k, v in out.items()}


def test_count_edges(env):
    """n in POOL_COUNTS: every kernel's first n rows are the first n rows of the n = 1025 result, nothing is written behind them;
    a permutation of the pool permutes the rows; n = 0 writes nothing"""
    L = env["L"]
    cam_np, bal_np = R.pool()
    assert len(cam_np) == R.POOL == max(R.POOL_COUNTS)
    cam, bal = _up(env, cam_np), _up(env, bal_np)
    rows = R.POOL + 64
    doubles = int(L.lib().c2b_camblk_doubles(R.POOL)) + 4096
    full = _run_four(env, cam, bal, R.POOL, rows, doubles)
    assert not np.any(full["from_bal"][:R.POOL] == CANARY) and not np.any(full["to_bal"][:R.POOL] == CANARY)
    for n in (0,) + R.POOL_COUNTS:
        got = _run_four(env, cam, bal, n, rows, doubles)
        for key in ("from_bal", "to_bal"):
            assert np.array_equal(got[key][:n], full[key][:n]), "%s: n = %d differs from the first rows of n = %d" % (key, n, R.POOL)
            assert np.all(got[key][n:] == CANARY), "%s: n = %d wrote behind row n" % (key, n)
        for form in ("state", "bal"):
            rec, flat, cen = got[form]
            assert rec.shape == (n, 32) and np.array_equal(rec, full[form][0][:n]), "prepare_%s: n = %d differs" % (form, n)
            assert np.array_equal(cen[:n], full[form][2][:n]) and np.all(cen[n:] == CANARY), "prepare_%s: cen4 at n = %d" % (form, n)
            assert np.all(flat[int(L.lib().c2b_camblk_doubles(n)):] == CANARY), "prepare_%s: n = %d wrote behind the table" % (form, n)
            assert not np.any(rec == CANARY)
    perm = np.random.default_rng(9).permutation(R.POOL)
    got = _run_four(env, _up(env, cam_np[perm]), _up(env, bal_np[perm]), R.POOL, rows, doubles)
    for key in ("from_bal", "to_bal"):
        assert np.array_equal(got[key][:R.POOL], full[key][:R.POOL][perm]), "%s: a camera's result depends on its place" % key
    for form in ("state", "bal"):
        assert np.array_equal(got[form][0], full[form][0][perm]) and np.array_equal(got[form][2][:R.POOL], full[form][2][:R.POOL][perm]), form


# ---- Level 1 runs the same kernels --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "angles"])
def test_level1_agrees_with_level0(env, fams, name):
    D, c2b = env["D"], env["c2b"]
    cam = fams[name]["cam15"]
    pts = np.zeros((1, 3))
    empty = (np.zeros(len(cam) + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2)))
    b0 = D.cameras_to_bal(_up(env, cam)).cpu().numpy()
    back = D.cameras_from_bal(_up(env, b0)).cpu().numpy()
    ba = c2b.BAProblem.from_visibility(cam, pts, *empty)
    assert _same(ba.cameras_bal(), b0), "%s: Level 1's cameras_bal is not device.cameras_to_bal" % name
    assert _same(ba.cameras(), cam)
    ba.apply_step(None, None)                                   # bal9 becomes the truth: to_vec, then the cameras rebuilt from it
    assert _same(ba.cameras(), back), "%s: apply_step with no step is not from_bal(to_bal(cameras))" % name
    assert _same(ba.cameras_bal(), b0)
    b = fams[name]["bal9"] if fams[name]["bal9"] is not None else b0
    want = D.cameras_from_bal(_up(env, b)).cpu().numpy()
    ba = c2b.BAProblem.from_bal(b, pts, *empty)
    assert _same(ba.cameras(), want), "%s: Level 1's from_bal is not device.cameras_from_bal" % name
    assert _same(ba.cameras_bal(), b)
