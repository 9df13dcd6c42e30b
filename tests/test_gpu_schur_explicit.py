"""The explicit Schur complement on the device (k_schur_y, k_schur_blocks_light / _heavy, k_schur_spmv,
k_const_offdiag; BAProblem.set_schur / schur_complement / schur_bytes, device.schur_*_rows, levenberg_marquardt*(schur=...))
against the longdouble reference of tests/_explicitref.py built from the device's own Jacobian: the blocks and the pattern, the
bit-exact transpose symmetry, the two paths at the edges of the LDS budget, the product, every PCG iterate, the stopping
iteration, the converged step, the untouched default path, the handle's state and the LM loop.  The tolerances are the
project's rule (16 x the largest deviation over 8 seeded perturbed reruns of the reference, floored at 1e-13 of the
absolute-value scale).  Worst |err| / bound seen on the MI355X (the EXPLICIT lines this prints): DESIGN 4.22."""
import ctypes as C

import numpy as np
import pytest

import _covisref as CR
import _explicitref as X
import _precondref as PR
import _robustref as B
import _schurref as R
import _solvecheck as SC
import oracle as O
from test_gpu_coupled import _dome, _lin, _load
from test_gpu_schur_jacobi import _device_blocks
from test_gpu_schur_step import EPS, _bits, _kappa, _level0, _make, _np, _ref, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
KINDS = ["block_jacobi", "schur_jacobi"]
_cache = {}


def _over(err, bound):
    return np.array([SC.over(e, b) for e, b in zip(err, bound)]) if len(err) else np.zeros(0)


def _norms(A):
    return np.linalg.norm(np.asarray(A, dtype=np.float64).reshape(len(A), -1), axis=1) if len(A) else np.zeros(0)


def _transposes_are_bit_exact(nbr_ptr, nbr, So):
    eid, row = X._edge_ids(nbr_ptr, nbr, len(nbr_ptr) - 1)
    back = eid[nbr.astype(np.int64), row]
    assert (back >= 0).all()
    return _bits(So, So[back].transpose(0, 2, 1))


def _check_system(ba, Q, lam, tag, runs=8):
    """ba.schur_complement(lam) against the reference of the longdouble problem Q: the pattern exactly, S_diag and S_off block
    by block in the Frobenius norm, b row by row (1e-12 of its scale, as the implicit passes that form it are held), the
    transposes bit for bit, two builds the same bytes.  Returns the device's arrays."""
    got = ba.schur_complement(lam)
    again = ba.schur_complement(lam)
    assert all(_bits(a, b) for a, b in zip(got, again)), (tag, "two builds differ")
    nbr_ptr, nbr, Sd, So, b = got
    ref = X.blocks_bound(Q, lam, runs=runs)
    assert _bits(nbr_ptr, ref["nbr_ptr"]) and _bits(nbr, ref["nbr"]), (tag, "pattern")
    assert Sd.shape == (Q.n_cam, 9, 9) and So.shape == (len(nbr), 9, 9) and b.shape == (Q.n_cam, 9)
    assert np.isfinite(Sd).all() and np.isfinite(So).all() and np.isfinite(b).all()
    ovD = _over(_norms(Sd - ref["D"].astype(np.float64)), ref["bound_D"])
    ovE = _over(_norms(So - ref["E"].astype(np.float64)), ref["bound_E"])
    want, scale = Q.rhs(lam)
    ovb = SC.rows_over((b.astype(R.LD) - want).astype(np.float64), scale, 1e-12) if Q.n_cam else np.zeros(0)
    worst = [float(v.max()) if len(v) else 0.0 for v in (ovD, ovE, ovb)]
    print("EXPLICIT blocks %s lam=%g n_cam=%d n_edges=%d worst |err|/bound: S_diag %.3g S_off %.3g b %.3g" % ((tag, lam, Q.n_cam, len(nbr)) + tuple(worst)))
    assert max(worst) <= 1.0, (tag, lam, worst, int(ovD.argmax()) if len(ovD) else -1, int(ovE.argmax()) if len(ovE) else -1)
    assert _transposes_are_bit_exact(nbr_ptr, nbr, So), (tag, "S_off[(c', c)] is not the transpose of S_off[(c, c')] bit for bit")
    return got


# ---- 1. the blocks on the dome ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bal", "state"])
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_blocks_on_the_dome(env, lam, mode):
    P = _dome(mode)
    ba = _load(P)
    Q = _lin(ba)
    assert PR.has_duplicate_pairs(Q)
    kc = np.diff(ba.row_ptr.astype(np.int64))
    assert (kc == 0).sum() == 1 and kc.max() == 257
    nbr_ptr, nbr, Sd, So, b = _check_system(ba, Q, lam, "dome " + mode)
    g = ba.covisibility(1)
    assert _bits(nbr_ptr, g[0]) and _bits(nbr, g[1])
    deg = np.diff(nbr_ptr.astype(np.int64))
    from city2ba_amd import device as D
    assert deg.max() == 79 > D.SCHUR_LDS_BLOCKS                  # the crowded point joins every pair: heavy rows (the light path: 3. below)
    assert _bits(Sd[kc == 0], np.diag(np.full(9, lam * 1e-6))[None])                              # an empty camera: the damping's diagonal
    assert ba.schur() == "implicit"                                                                # the entry leaves the setting alone
    assert ba.schur_bytes() == 8 * (81 * (len(nbr) + len(Sd)) + 27 * ba.num_observations())
    ba.close()


def test_duplicated_pairs_reach_the_diagonal(env):
    """S_diag is S's own diagonal, not the Schur-Jacobi M: where a pair repeats the two differ by more than both bounds"""
    P = _dome("bal")
    ba = _load(P)
    Q = _lin(ba)
    lam = 1e-2
    Sd = ba.schur_complement(lam)[2]
    M = _device_blocks(env, ba, True, lam)
    ref = X.blocks_bound(Q, lam, runs=2)
    _, mb, _ = PR.blocks_bound(Q, lam, runs=2)
    gap = _norms(Sd - M)
    key = np.sort(Q.cam * Q.n_pts + Q.pt)
    dup_cams = np.unique(key[1:][np.diff(key) == 0] // Q.n_pts)         # the cameras with a repeated (camera, point) pair
    assert len(dup_cams) and (gap[dup_cams] > ref["bound_D"][dup_cams] + mb[dup_cams]).all()
    rest = np.setdiff1d(np.arange(Q.n_cam), dup_cams)
    assert (gap[rest] <= ref["bound_D"][rest] + mb[rest]).all()
    ba.close()


# ---- 2. the block-diagonal case -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_block_diagonal_problem(env, lam):
    ba, bal = _make("random bal")
    Q = _ref(ba, R.LD)
    assert len(np.unique(Q.pt)) == len(Q.pt)                     # every point seen once
    nbr_ptr, nbr, Sd, So, b = _check_system(ba, Q, lam, "random bal")
    assert len(nbr) == 0 and not nbr_ptr.any() and So.shape == (0, 9, 9)
    M = _device_blocks(env, ba, bal, lam)
    _, mb, _ = PR.blocks_bound(Q, lam, runs=8)
    ref = X.blocks_bound(Q, lam, runs=8)
    assert (_norms(Sd - M) <= mb + ref["bound_D"]).all()         # S_diag is the Schur-Jacobi M within both bounds
    ba.set_schur("explicit")
    ba.set_preconditioner("schur_jacobi")
    pref = X.pcg(Q, lam, 1, 0.0, kind="schur_jacobi", runs=8)
    SC.check_iterates(ba, Q, pref, lam, (0, 1), tag="random bal explicit", label="EXPLICIT iterates")
    tol = min(float(pref["rel"][1]) + pref["bound"]["rel"][1], float(np.sqrt(R.EPS)))
    _, _, info = ba.solve_step(lam, max_iters=50, rel_tol=tol)
    assert info["status"] == 0 and info["iterations"] == 1 and info["rel_residual"] <= tol, (lam, tol, info)
    ba.close()


# ---- 3. the edges of the two paths --------------------------------------------------------------------------------------------
def _list_problem(row_ptr, pt_idx, n_pts, seed=0):
    """a bal-mode problem on a given list: the dome's construction -- cameras on a shell of radius 8-14 looking at the origin with a
    random roll, points in the box [-2, 2]^3, so every point is in front of every camera -- observations the oracle's
    projection + 1e-3, the state moved by 1e-3"""
    import city2ba_amd as c2b
    rng = np.random.default_rng(seed)
    n_cam = len(row_ptr) - 1
    pts = rng.uniform(-2.0, 2.0, size=(n_pts, 3))
    cams = np.empty((n_cam, 15))
    for c in range(n_cam):
        d = rng.normal(size=3)
        ctr = d / np.linalg.norm(d) * rng.uniform(8.0, 14.0)
        z = ctr / np.linalg.norm(ctr)
        a = np.cross(z, rng.normal(size=3))
        x = a / np.linalg.norm(a)
        Rm = np.stack([x, np.cross(z, x), z])
        cams[c, :9] = Rm.T.ravel()
        cams[c, 9:12] = -Rm @ ctr
    cams[:, 12] = rng.uniform(0.8, 1.2, n_cam)
    cams[:, 13:15] = rng.uniform(-5e-2, 5e-2, size=(n_cam, 2))
    bal9 = O.camera_to_bal(cams)
    row_ptr, pt_idx = np.asarray(row_ptr, dtype=np.uint64), np.asarray(pt_idx, dtype=np.uint64)
    uv = O.project_observations(O.camera_from_bal(bal9), pts, row_ptr, pt_idx) if len(pt_idx) else np.zeros((0, 2))
    uv = uv + rng.normal(scale=1e-3, size=uv.shape)
    bal9[:, :6] += rng.normal(scale=1e-3, size=(n_cam, 6))
    pts = pts + rng.normal(scale=1e-3, size=pts.shape)
    return c2b.BAProblem.from_bal(bal9, pts, row_ptr, pt_idx, uv, device=0)


def _edge_cases():
    from_header = 32                                             # C2B_SCHUR_LDS_BLOCKS (asserted against the binding below)
    Bk = from_header
    cases = [("hub %d" % d, d, False) for d in (1, 63, 64, 65, Bk - 1, Bk, Bk + 1, 3 * Bk)]
    cases += [("tight hub %d" % d, d, True) for d in (Bk, Bk + 1, 65)]
    return Bk, cases


@pytest.mark.parametrize("which", [c[0] for c in _edge_cases()[1]] + ["heavy only"])
def test_rows_at_the_edges_of_the_lds_budget(env, which):
    from city2ba_amd import device as D
    Bk, cases = _edge_cases()
    assert Bk == D.SCHUR_LDS_BLOCKS
    if which == "heavy only":
        row_ptr, pt_idx, n_pts = CR.heavy_only_list(2 * Bk)
        degree = 2 * Bk - 1
    else:
        _, degree, tight = [c for c in cases if c[0] == which][0]
        row_ptr, pt_idx, n_pts = CR.hub_list(degree, tight)
    ba = _list_problem(row_ptr, pt_idx, n_pts, seed=degree)
    Q = _ref(ba, R.LD)
    nbr_ptr, nbr, Sd, So, b = _check_system(ba, Q, 1e-2, which)
    deg = np.diff(nbr_ptr.astype(np.int64))
    assert deg[0] == degree and deg.max() == degree
    ba.close()


# ---- 4. empty and tiny ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["no observation", "one camera", "two cameras one point", "duplicates on both sides"])
def test_empty_and_tiny_lists(env, which):
    rows = {"no observation": [[], [], []], "one camera": [[0, 1, 2, 1]], "two cameras one point": [[0, 1, 2, 3], [4, 0, 5, 6]],
            "duplicates on both sides": [[1, 0, 2, 0, 3], [0, 4, 5, 0, 6, 0]]}[which]
    row_ptr, pt_idx = CR._lists(rows)
    n_pts = 7
    ba = _list_problem(row_ptr, pt_idx, n_pts, seed=len(which))
    lam = 1e-2
    if which == "no observation":
        nbr_ptr, nbr, Sd, So, b = ba.schur_complement(lam)
        assert not nbr_ptr.any() and len(nbr) == 0 and not b.any()
        assert _bits(Sd, np.broadcast_to(np.diag(np.full(9, lam * 1e-6)), (3, 9, 9)))
        ba.set_schur("explicit")
        dc, dp, info = ba.solve_step(lam)
        assert not _np(dc).any() and not _np(dp).any() and info["iterations"] == 0 and info["status"] == 0
    else:
        Q = _ref(ba, R.LD)
        nbr_ptr, nbr, Sd, So, b = _check_system(ba, Q, lam, which)
        assert len(nbr) == {"one camera": 0, "two cameras one point": 2, "duplicates on both sides": 2}[which]
        ba.set_schur("explicit")
        ks = (0, 1, 2)
        SC.check_iterates(ba, Q, X.pcg(Q, lam, max(ks), 0.0, runs=8), lam, ks, tag=which, label="EXPLICIT iterates")
    ba.close()


# ---- 5. the product ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dome", "random bal", "tight hub"])
def test_product_with_the_stored_blocks(env, name):
    """device.schur_spmv_rows against the longdouble product of the device's own blocks.  A row's sum has 9 (degree + 1) products:
    the rule's perturbed rerun moves it by eps of its absolute-value scale, 16 x that lies under the floor, so the bound is
    the floor, 1e-13 of the scale, row by row; the partials' sum is held the same way to x^T y."""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    if name == "dome":
        ba = _load(_dome("bal"))
    elif name == "random bal":
        ba = _make(name)[0]
    else:
        ba = _list_problem(*CR.hub_list(65, True), seed=2)
    nbr_ptr, nbr, Sd, So, _ = ba.schur_complement(1e-2)
    nc = len(Sd)
    x = np.random.default_rng(11).normal(size=(nc, 9))
    want, scale = X.spmv(nbr_ptr, nbr, Sd.astype(R.LD), So.astype(R.LD), x.astype(R.LD))
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else a.view(dt))).to(dev)
    d_ptr, d_nbr = t(nbr_ptr, np.int64), t(nbr if len(nbr) else np.zeros(1, dtype=np.uint32), np.int32)
    d_Sd, d_So, d_x = t(Sd), t(So if len(So) else np.zeros((1, 9, 9))), t(x)
    n_part = 4 * ((nc + 3) // 4)
    outs = []
    for part in (None, torch.full((n_part,), float("nan"), dtype=torch.float64, device=dev)):
        y = torch.full((nc, 9), float("nan"), dtype=torch.float64, device=dev)
        D.schur_spmv_rows(d_ptr, d_nbr, d_Sd, d_So, d_x, y, part)
        torch.cuda.synchronize()
        outs.append(_np(y).copy())
        ov = SC.rows_over((outs[-1].astype(R.LD) - want).astype(np.float64), scale, 1e-13)
        print("EXPLICIT spmv %s dot=%s worst |err|/bound %.3g" % (name, part is not None, float(ov.max())))
        assert float(ov.max()) <= 1.0, (name, int(ov.argmax()))
        if part is not None:
            got = _np(part)
            assert np.isfinite(got).all()
            xy = np.sum(x.astype(R.LD) * want)
            assert abs(float(np.sum(got.astype(R.LD)) - xy)) <= 1e-13 * float(np.sum(np.abs(x) * scale.astype(np.float64))), name
    assert _bits(outs[0], outs[1])                               # both instances: the same y
    ba.close()


def test_level0_passes_build_the_same_blocks(env):
    """device.schur_y_rows + schur_jacobi_blocks + schur_blocks_rows on the dome's own arrays give schur_complement's bytes"""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    ba = _load(_dome("bal"))
    lam = 1e-2
    nbr_ptr, nbr, Sd, So, _ = ba.schur_complement(lam)
    camblk, pts4, rows, prows, pi, uv = _level0(env, ba, True)
    f64 = dict(dtype=torch.float64, device=dev)
    nc, npt, no = ba.num_cameras(), ba.num_points(), ba.num_observations()
    U, gc, V, gp = torch.empty((nc, 9, 9), **f64), torch.empty((nc, 9), **f64), torch.empty((npt, 3, 3), **f64), torch.empty((npt, 3), **f64)
    D.normal_cameras_rows(camblk, pts4, rows, pi, uv, U, gc)
    D.normal_points_rows(camblk, pts4, prows, uv, V, gp)
    g_ptr, g_nbr, _ = D.covisibility_rows(rows, pi, prows, 1)
    assert _bits(_np(g_ptr).view(np.uint64), nbr_ptr) and _bits(_np(g_nbr).view(np.uint32), nbr)
    Y = torch.full((no, 3, 9), float("nan"), **f64)
    D.schur_y_rows(camblk, pts4, D.expand_rows(rows.row_ptr, no), pi, uv, V, lam, Y)
    M = torch.empty((nc, 9, 9), **f64)
    D.schur_jacobi_blocks(camblk, pts4, rows, pi, uv, U, V, lam, M)
    S_off = torch.full((len(nbr), 9, 9), float("nan"), **f64)
    D.schur_blocks_rows(rows, pi, prows, g_ptr, g_nbr, Y, M, S_off)
    torch.cuda.synchronize()
    assert _bits(_np(M), Sd) and _bits(_np(S_off), So)
    # W_o V_l^-1 W_o^T = Y_o^T Y_o, observation by observation
    Q = _lin(ba)
    Vi = R.inv3(Q.Vl(lam))[Q.pt]
    want = np.einsum("nab,nbc,ndc->nad", Q.W, Vi, Q.W)
    got = np.einsum("nka,nkb->nab", _np(Y).astype(R.LD), _np(Y).astype(R.LD))
    sc = np.einsum("nab,nbc,ndc->nad", np.abs(Q.W), np.abs(Vi), np.abs(Q.W))
    assert (_norms(got - want) <= 1e-12 * _norms(sc)).all()
    ba.close()


# ---- 6. the PCG ---------------------------------------------------------------------------------------------------------------
def _explicit_reference(key, ba, lam, ks, kind, loss=None, mask=None, runs=8):
    key = ("xref",) + key
    if key not in _cache:
        Q = _lin(ba, loss=loss, mask=mask)
        _cache[key] = (Q, X.pcg(Q, lam, max(ks), 0.0, kind=kind, runs=runs))
    return _cache[key]


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("kind", KINDS)
def test_pcg_iterates_on_the_dome(env, kind, lam):
    ba = _load(_dome("bal"))
    ba.set_schur("explicit")
    ba.set_preconditioner(kind)
    ks = SC.DOME_KS[(kind, lam)]
    Q, ref = _explicit_reference(("dome", kind, lam), ba, lam, ks, kind)
    SC.check_iterates(ba, Q, ref, lam, ks, tag="dome explicit " + kind, label="EXPLICIT iterates")
    assert ba.preconditioner_fallbacks() == 0
    if lam == 1e-4:                                              # the stopping iteration is the reference's
        tols = SC.crossing_tols(ref, 4)
        assert len(tols) >= 3, ref["rel"]
        for K, tol in tols:
            _, _, info = ba.solve_step(lam, max_iters=200, rel_tol=tol)
            assert info["status"] == 0 and info["iterations"] == K and info["rel_residual"] <= tol, (kind, K, tol, info)
    ba.close()


def _issue_grid_on_the_device():
    """_precondref.issue_grid's construction (2 blocks: 240 cameras, 720 points), loaded in bal mode"""
    import city2ba_amd as c2b
    from _problems import grid_candidate_pairs, grid_cameras_points
    cams15, pts = grid_cameras_points(2)
    cam_idx, pt_idx = grid_candidate_pairs(cams15, pts, 10.0)
    Rm = cams15[cam_idx, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    qz = np.einsum("nj,nj->n", Rm[:, 2, :], pts[pt_idx]) + cams15[cam_idx, 11]
    keep = qz <= -0.5
    cam_idx, pt_idx = cam_idx[keep].astype(np.int64), pt_idx[keep].astype(np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam_idx, minlength=len(cams15)))]).astype(np.uint64)
    rng = np.random.default_rng(0)
    uv = O.project_observations(cams15, pts, row_ptr, pt_idx) + rng.normal(scale=1e-3, size=(len(pt_idx), 2))
    bal9 = O.camera_to_bal(cams15)
    bal9[:, :6] += rng.normal(scale=1e-2, size=(len(cams15), 6))
    pts = pts + rng.normal(scale=1e-2, size=pts.shape)
    return c2b.BAProblem.from_bal(bal9, pts, row_ptr, pt_idx.astype(np.uint64), uv, device=0)


@pytest.mark.parametrize("kind", KINDS)
def test_pcg_iterates_on_the_issue_grid(env, kind):
    ba = _issue_grid_on_the_device()
    assert (ba.num_cameras(), ba.num_points()) == (240, 720)
    ba.set_schur("explicit")
    ba.set_preconditioner(kind)
    lam, ks = 1e-2, SC.DOME_KS_SHORT
    Q = _ref(ba, R.LD)
    SC.check_iterates(ba, Q, X.pcg(Q, lam, max(ks), 0.0, kind=kind, runs=3), lam, ks, tag="issue grid explicit " + kind, label="EXPLICIT iterates")
    ba.close()


@pytest.mark.parametrize("kind", KINDS)
def test_pcg_iterates_under_cauchy(env, kind):
    P = _dome("bal")
    lam, ks = 1e-2, SC.DOME_KS_SHORT
    uv, _ = SC.dome_scaled_observations(P)
    ba = _load(P, uv)
    a = SC.cauchy_scale(ba.residual_jacobian()[0])
    ba.set_loss("cauchy", a)
    ba.set_schur("explicit")
    ba.set_preconditioner(kind)
    Q, ref = _explicit_reference(("cauchy", kind), ba, lam, ks, kind, loss=("cauchy", a))
    SC.check_iterates(ba, Q, ref, lam, ks, tag="dome explicit cauchy " + kind, label="EXPLICIT iterates")
    if kind == KINDS[0]:                                         # (the blocks do not depend on the preconditioner: once)
        _check_system(ba, Q, lam, "dome cauchy")
    ba.close()


@pytest.mark.parametrize("kind", KINDS)
def test_pcg_iterates_under_a_mask(env, kind):
    """constant entries are exact zeros at every iterate, the blocks are those of J~"""
    P = _dome("bal")
    lam, ks = 1e-2, SC.DOME_KS_SHORT
    ba = _load(P)
    cm, pm = SC.dome_mask(P)
    ba.set_schur("explicit")
    ba.set_preconditioner(kind)
    ba.set_constant(cm, pm)
    Q, ref = _explicit_reference(("mask", kind), ba, lam, ks, kind, mask=(cm, pm))
    SC.check_iterates(ba, Q, ref, lam, ks, tag="dome explicit mask " + kind, label="EXPLICIT iterates")
    for k in ks:
        dc, dp, _ = ba.solve_step(lam, max_iters=k, rel_tol=0.0)
        SC.assert_zeros(_np(dc), _np(dp), cm, pm, ("explicit mask", kind, k))
    nbr_ptr, nbr, Sd, So, b = _check_system(ba, Q, lam, "dome mask") if kind == KINDS[0] else ba.schur_complement(lam)
    m = SC.unpack(cm)
    row = np.repeat(np.arange(len(cm)), np.diff(nbr_ptr.astype(np.int64)))
    assert not So[m[row]].any() and not So.transpose(0, 2, 1)[m[nbr.astype(np.int64)]].any()         # constant rows and columns: 0
    off = Sd.copy()
    i = np.arange(9)
    assert _bits(Sd[:, i, i][m], np.full(int(m.sum()), lam * 1e-6))                                 # a constant diagonal entry
    off[:, i, i] = 0.0
    assert not off[m].any() and not off.transpose(0, 2, 1)[m].any() and not b[m].any()
    ba.close()


def test_converged_step_agrees_with_the_implicit_path_and_the_dense_solve(env):
    """test_converged_step_agrees_with_block_jacobi's rule between the two paths: at rel_tol both reach, the device steps may differ
    by what the two references' converged solutions differ by plus each one's own bound; and test_gpu_coupled's criteria against
    the dense direct solve on the dome."""
    ba, _ = _make("small grid culled")
    Q = _ref(ba, R.LD)
    lam, tol = 1e-2, 1e-10
    ri = PR.pcg(Q, lam, 400, tol, kind="block_jacobi", runs=3)
    re = X.pcg(Q, lam, 400, tol, kind="block_jacobi", runs=3)
    assert ri["status"] == 0 and re["status"] == 0
    dci, dpi, ii = ba.solve_step(lam, max_iters=400, rel_tol=tol)
    dci, dpi = _np(dci).copy(), _np(dpi).copy()
    ba.set_schur("explicit")
    dce, dpe, ie = ba.solve_step(lam, max_iters=400, rel_tol=tol)
    dce, dpe = _np(dce), _np(dpe)
    assert ii["status"] == 0 and ie["status"] == 0, (ii, ie)
    for key, gi, ge in (("x", dci, dce), ("dp", dpi, dpe)):
        gap = float(np.linalg.norm((ri[key][-1] - re[key][-1]).astype(np.float64)))
        bound = gap + ri["bound"][key][-1] + re["bound"][key][-1]
        err = float(np.linalg.norm(gi - ge))
        print("EXPLICIT step agreement %s: |implicit - explicit| %.3g, bound %.3g (reference gap %.3g), iterations %d vs %d"
              % (key, err, bound, gap, ii["iterations"], ie["iterations"]))
        assert err <= bound, (key, err, bound)
    ba.close()
    for lam in (1e-4, 1.0):
        ba = _load(_dome("bal"))
        ba.set_schur("explicit")
        ba.set_preconditioner("schur_jacobi")
        ref = _lin(ba, np.float64)
        dc, dp, info = ba.solve_step(lam, max_iters=5000, rel_tol=1e-12)
        dc, dp = _np(dc), _np(dp)
        assert info["status"] == 0 and info["rel_residual"] <= 1e-12, info
        kappa = _kappa(ref, lam)
        tol_res = max(1e-9, 1e3 * EPS * kappa)
        res, g = ref.damped_residual(lam, dc, dp)
        wc, wp = ref.schur_direct(lam)
        d, w = np.concatenate([dc.ravel(), dp.ravel()]), np.concatenate([wc.ravel(), wp.ravel()])
        print("EXPLICIT dense lam=%g: kappa %.3g, %d iterations, |res| / |g| %.3g, |d - w| / |w| %.3g"
              % (lam, kappa, info["iterations"], np.linalg.norm(res) / np.linalg.norm(g), np.linalg.norm(d - w) / np.linalg.norm(w)))
        assert np.linalg.norm(res) <= tol_res * np.linalg.norm(g), (lam, kappa)
        assert np.linalg.norm(d - w) <= max(1e-8, kappa * tol_res) * np.linalg.norm(w), (lam, kappa)
        ba.close()


# ---- 7. priors ----------------------------------------------------------------------------------------------------------------
def test_step_under_priors_equals_the_implicit_step(env):
    """test_converged_step_agrees_with_block_jacobi's rule on the stacked system (the device's own prior rows appended as
    pseudo-observations): at rel_tol both reach, the device steps may differ by what the two references' converged solutions
    differ by plus each one's own bound."""
    from test_gpu_priors import _stacked, _with_priors
    ba, bal, kw = _with_priors("small grid culled")
    lam, tol = 1e-2, 1e-10
    Q = _stacked(ba, kw, dtype=R.LD)
    ri = PR.pcg(Q, lam, 400, tol, kind="block_jacobi", runs=3)
    re = X.pcg(Q, lam, 400, tol, kind="block_jacobi", runs=3)
    assert ri["status"] == 0 and re["status"] == 0
    dci, dpi, ii = ba.solve_step(lam, max_iters=400, rel_tol=tol)
    dci, dpi = _np(dci).copy(), _np(dpi).copy()
    ba.set_schur("explicit")
    dce, dpe, ie = ba.solve_step(lam, max_iters=400, rel_tol=tol)
    assert ii["status"] == 0 and ie["status"] == 0 and not _bits(dci, _np(dce)), (ii, ie)
    for key, gi, ge in (("x", dci, _np(dce)), ("dp", dpi, _np(dpe))):
        gap = float(np.linalg.norm((ri[key][-1] - re[key][-1]).astype(np.float64)))
        bound = gap + ri["bound"][key][-1] + re["bound"][key][-1]
        err = float(np.linalg.norm(gi - ge))
        print("EXPLICIT priors %s: |implicit - explicit| %.3g, bound %.3g (reference gap %.3g), iterations %d vs %d"
              % (key, err, bound, gap, ii["iterations"], ie["iterations"]))
        assert err <= bound, (key, err, bound)
    ba.close()


# ---- 8. the untouched default; refusals ---------------------------------------------------------------------------------------
def test_default_path_is_untouched_and_the_solve_is_deterministic(env):
    lam = 1e-4
    plain, _ = _make("small grid culled")
    want = plain.solve_step(lam, max_iters=7, rel_tol=0.0)
    want = [_np(want[0]).copy(), _np(want[1]).copy(), want[2]]
    assert plain.schur() == "implicit"
    plain.close()
    ba, _ = _make("small grid culled")
    ba.set_schur("explicit")
    assert ba.schur() == "explicit"
    a = ba.solve_step(lam, max_iters=7, rel_tol=0.0)
    a = [_np(a[0]).copy(), _np(a[1]).copy(), a[2]]
    b = ba.solve_step(lam, max_iters=7, rel_tol=0.0)
    assert _bits(a[0], _np(b[0])) and _bits(a[1], _np(b[1])) and a[2] == b[2]      # the same bits twice
    assert not _bits(a[0], want[0])
    ba.set_schur("implicit")
    got = ba.solve_step(lam, max_iters=7, rel_tol=0.0)
    assert _bits(_np(got[0]), want[0]) and _bits(_np(got[1]), want[1]) and got[2] == want[2]       # a handle that never had it set
    with pytest.raises(ValueError):
        ba.set_schur("dense")
    from city2ba_amd import _lib as L
    with pytest.raises(L.City2baError):
        ba.set_schur(2)
    assert ba.schur() == "implicit"
    lib = L.lib()
    n = C.c_int64(-7)
    L.check(lib.c2b_problem_set_shard(ba._h, 0, 2 * ba.num_cameras(), 0))
    ba.set_schur("explicit")
    dummy = (C.c_double * 8)()
    for rc in (lib.c2b_problem_schur_bytes(ba._h, C.byref(n)), lib.c2b_problem_get_schur_pattern(ba._h, None, None),
               lib.c2b_problem_schur_complement(ba._h, 1e-2, dummy, dummy, dummy, C.byref(n))):
        assert rc == L.ERR_INVALID_ARGUMENT and b"shard" in lib.c2b_last_error() and n.value == -7
    ba.close()
    import city2ba_amd as c2b
    empty = c2b.BAProblem(0)
    assert lib.c2b_problem_schur_bytes(empty._h, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"nothing uploaded" in lib.c2b_last_error()
    assert lib.c2b_problem_schur_complement(empty._h, 1e-2, dummy, dummy, dummy, C.byref(n)) == L.ERR_INVALID_ARGUMENT and n.value == -7
    assert lib.c2b_problem_schur_complement(empty._h, 0.0, dummy, dummy, dummy, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"lambda" in lib.c2b_last_error()
    empty.set_schur("explicit")                                  # the handle's, with or without an upload
    assert empty.schur() == "explicit"
    empty.close()


# ---- 9. the handle's state ------------------------------------------------------------------------------------------------------
def test_setting_survives_upload_and_cull_and_is_carried_by_a_window(env):
    from test_gpu_schur_step import _grid
    g = _grid(cull=False)
    g.set_schur("explicit")
    g.cull()
    assert g.schur() == "explicit"
    bal9, pts, rp, pi, uv = g.cameras_bal(), g.points(), g.row_ptr.copy(), g.pt_idx.copy(), g.observations()
    uv = uv + np.random.default_rng(3).normal(scale=1e-2, size=uv.shape)
    g._upload(bal9, True, pts, rp, pi, uv)
    assert g.schur() == "explicit"
    _, _, info = g.solve_step(1e-2, max_iters=3, rel_tol=0.0)
    assert info["iterations"] == 3
    w = g.window(range(5))
    assert w.schur() == "explicit"
    _, _, info = w.solve_step(1e-2, max_iters=3, rel_tol=0.0)
    assert info["iterations"] == 3
    w.close()
    for carry, want in ((False, "implicit"), (True, "explicit")):    # without carry: a new problem's
        child = g.subset(np.arange(4), np.arange(g.num_points()), carry=carry)
        assert child.schur() == want
        child.close()
    g.close()


def test_pattern_and_blocks_follow_the_list(env):
    """kept across apply_step, rollback and covisibility(5) (the solver's pattern is its own copy at threshold 1); rebuilt after
    what changes the list"""
    P = _dome("bal")
    ba = _load(P)
    lam = 1e-2
    ba.set_schur("explicit")
    first = ba.schur_complement(lam)
    g5 = ba.covisibility(5)
    assert len(g5[1]) < len(first[1])
    assert all(_bits(a, b) for a, b in zip(first, ba.schur_complement(lam)))                   # another threshold cached: S as it was
    dc, dp, _ = ba.solve_step(lam, max_iters=3, rel_tol=0.0)
    ba.checkpoint()
    ba.apply_step(dc, dp)
    moved = ba.schur_complement(lam)
    assert _bits(moved[0], first[0]) and _bits(moved[1], first[1]) and not _bits(moved[2], first[2])
    ba.rollback()
    assert all(_bits(a, b) for a, b in zip(first, ba.schur_complement(lam)))                   # the state and the pattern are back
    assert ba.filter_observations(2e-3) > 0                      # the list changes: the pattern is the new list's
    after = ba.schur_complement(lam)
    want = CR.graph(ba.row_ptr, ba.pt_idx, 1)
    assert _bits(after[0], want[0]) and _bits(after[1], want[1]) and len(after[1]) < len(first[1])
    _, _, info = ba.solve_step(lam, max_iters=3, rel_tol=0.0)
    assert info["iterations"] == 3
    ba.close()


def test_fifty_rounds_leave_the_free_memory_where_it_was(env):
    """in the manner of tests/test_gpu_covisibility.py: a warm-up round, then 50 rounds of set / solve / drop (a filter that
    removes one observation drops the rows, the pattern and the solve buffers)"""
    torch = env["torch"]
    ba = _load(_dome("bal"))
    bal9, pts, rp, pi, uv = ba.cameras_bal(), ba.points(), ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations()

    def round_():
        ba.set_schur("explicit")
        ba.solve_step(1e-2, max_iters=2, rel_tol=0.0)
        ba.schur_complement(1e-2)
        ba.set_schur("implicit")
        ba._upload(bal9, True, pts, rp, pi, uv)                  # drops the rows, the transpose, the solve buffers and the pattern
    round_()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(50):
        round_()
    torch.cuda.synchronize()
    drop = free0 - torch.cuda.mem_get_info(0)[0]
    print("free device memory dropped by %d bytes over 50 explicit set / solve / drop rounds" % drop)
    assert drop <= 0
    ba.close()


# ---- 10. the LM loop ----------------------------------------------------------------------------------------------------------
def test_lm_loop_reaches_the_implicit_loop_s_error(env):
    """test_gpu_schur_jacobi.test_lm_loop_...'s allowance, between the two paths: both loops solve every step to rel_tol 1e-10; the
    two references' converged solutions of the first linearisation differ by a relative eta in the step (their gap plus each
    one's bound, floored at 1e-13), and the final errors are held to 16 x iterations x 2 eta, relative."""
    from city2ba_amd.solve import levenberg_marquardt_device
    its, lam, tol = 6, 1e-4, 1e-10
    out = {}
    for schur in ("implicit", "explicit"):
        ba, _ = _make("small grid culled")
        if schur == "implicit":
            Q = _ref(ba, R.LD)
            ri = PR.pcg(Q, lam, 3000, tol, kind="schur_jacobi", runs=1)
            re = X.pcg(Q, lam, 3000, tol, kind="schur_jacobi", runs=1)
            assert ri["status"] == 0 and re["status"] == 0
            gap = float(np.linalg.norm((ri["x"][-1] - re["x"][-1]).astype(np.float64))) + ri["bound"]["x"][-1] + re["bound"]["x"][-1]
            eta = max(gap / float(np.linalg.norm(ri["x"][-1].astype(np.float64))), 1e-13)
        hist, summary = levenberg_marquardt_device(ba, its, lam=lam, max_iters=3000, rel_tol=tol, preconditioner="schur_jacobi", schur=schur)
        assert ba.schur() == schur and all(h["status"] == 0 for h in hist), [(h["status"], h["pcg_iterations"]) for h in hist]
        out[schur] = (hist[-1]["error_after"], [h["accepted"] for h in hist], sum(h["pcg_iterations"] for h in hist))
        ba.close()
    (ei, ai, ni), (ee, ae, ne) = out["implicit"], out["explicit"]
    bound = 16 * its * 2 * eta
    print("EXPLICIT lm: final error %.15g (implicit, %d PCG iterations) %.15g (explicit, %d); |diff| / error %.3g, bound %.3g"
          % (ei, ni, ee, ne, abs(ei - ee) / ei, bound))
    assert ai == ae and abs(ei - ee) <= bound * ei, (ei, ee, bound, ai, ae)
