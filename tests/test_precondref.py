"""The Schur-Jacobi preconditioner's host reference (tests/_precondref.py) checked on the CPU: its blocks are the diagonal
blocks of S when no camera sees a point twice and stay positive definite when one does; on the grid the two
preconditioners were compared on it at least halves the reference's iteration count; the built library exports the new
entries under a new ABI number.  (That the weighted pass is the one text of k_schur_jacobi plus one line is
tests/test_robust_loss_fold.py's, with the other five passes.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _precondref as PR
import _schurref as R

LD = R.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELD = float(np.finfo(LD).eps)


def _random(seed, n_cam=12, n_pts=40, n_obs=160, dtype=LD):
    """random r / Jc / Jp (uneven columns like f, k1, k2) on a list without a repeated (camera, point) pair; camera 0 empty"""
    rng = np.random.default_rng(seed)
    pairs = rng.choice((n_cam - 1) * n_pts, n_obs, replace=False)
    pairs.sort()
    cam_of, pt_idx = 1 + pairs // n_pts, pairs % n_pts
    scale = np.array([1.0, 1.0, 1.0, 0.1, 0.1, 0.1, 1e-3, 10.0, 100.0])
    return R.Problem(rng.normal(size=(n_obs, 2)), rng.normal(size=(n_obs, 2, 9)) * scale, rng.normal(size=(n_obs, 2, 3)),
                     cam_of, pt_idx, n_cam, n_pts, dtype=dtype)


def _over(err, bound):
    """|err| / bound per entry; an entry whose scale is 0 (an empty camera's off-diagonal) must be exact"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


@pytest.fixture(scope="module")
def grid():
    import __graft_entry__ as entry
    entry.build()                                                # the oracle's library
    P = PR.issue_grid(2, dtype=LD)
    assert (P.n_cam, P.n_pts) == (240, 720) and not PR.has_duplicate_pairs(P)
    return P


# ---- 1. unique pairs: the blocks are S's diagonal blocks ------------------------------------------------------------------
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_blocks_are_the_schur_complements_diagonal_blocks(grid, lam):
    """Both sides are the same numbers by algebra; each is a sum of at most a few hundred longdouble products whose
    absolute values add up to SM and SD, so they may differ by that many roundings of (SM + SD): 512 eps of longdouble
    per entry.  Problem.dense_S inverts V_l in f64, which SD's |V^-1| SV |V^-1| term covers at f64's eps."""
    for P in (grid, _random(7)):
        M, SM = PR.blocks(P, lam)
        D, SD = PR.schur_diag_blocks(P, lam)
        over = _over(np.abs(M - D), 512 * ELD * (SM + SD))
        assert float(over.max()) <= 1.0, (lam, float(over.max()))
        assert float(_over(np.abs(M - M.transpose(0, 2, 1)), 512 * ELD * SM).max()) <= 1.0
        S = P.dense_S(lam)
        Sd = np.stack([S[9 * c:9 * c + 9, 9 * c:9 * c + 9] for c in range(P.n_cam)])
        over64 = _over(np.abs(M.astype(np.float64) - Sd), 512 * R.EPS * (SM + SD))
        print("PRECONDREF lam=%g n_cam=%d worst |M - S_cc| over its bound: longdouble %.3g, dense_S (f64) %.3g"
              % (lam, P.n_cam, float(over.max()), float(over64.max())))
        assert float(over64.max()) <= 1.0, (lam, float(over64.max()))


def test_an_empty_camera_gets_the_dampings_diagonal():
    P = _random(8)
    M, _ = PR.blocks(P, 1e-3)
    assert np.array_equal(M[0].astype(np.float64), np.diag(np.full(9, 1e-3 * 1e-6)))


# ---- 2. a duplicated pair: no longer S's block, still positive definite ------------------------------------------------
@pytest.mark.parametrize("lam", [1e-12, 1e-4, 1.0])
def test_duplicated_pair_differs_from_s_but_keeps_positive_pivots(lam):
    P0 = _random(9)
    cam, pt = P0.cam.copy(), P0.pt.copy()
    c = cam[5]
    assert cam[6] == c                                           # two observations of one camera ...
    pt[6] = pt[5]                                                # ... now of one point
    P = R.Problem(P0.r, P0.Jc, P0.Jp, cam, pt, P0.n_cam, P0.n_pts, dtype=LD)
    assert PR.has_duplicate_pairs(P)
    M, SM = PR.blocks(P, lam)
    D, SD = PR.schur_diag_blocks(P, lam)
    over = _over(np.abs(M - D), 512 * ELD * (SM + SD))
    others = np.arange(P.n_cam) != c
    piv = PR.pivots(M)
    assert np.isfinite(piv.astype(np.float64)).all() and (piv > 0).all(), float(piv.min())
    assert float(over[others].max()) <= 1.0, float(over[others].max())
    if lam < 1e-4:                                               # points seen once: |V_l^-1| ~ 1 / lam swamps the scale of S_cc
        return
    assert float(over[c].max()) > 1e6, float(over[c].max())
    # M_c - S_cc is the cross terms 2 sym(W_5 V^-1 W_6^T) that the per-observation definition leaves out
    Vi = R.inv3(P.Vl(lam))[pt[5]]
    X = P.W[5] @ Vi @ P.W[6].T
    assert np.abs((M[c] - D[c]) - (X + X.T)).max() <= 512 * ELD * float((SM[c] + SD[c]).max())


# ---- 3. what it buys, on the reference ---------------------------------------------------------------------------------
def test_schur_jacobi_at_least_halves_the_iterations_on_the_grid(grid):
    lam, tol = 1e-4, 1e-2
    bj = PR.pcg_plain(grid, lam, 400, tol, kind="block_jacobi")
    sj = PR.pcg_plain(grid, lam, 400, tol, kind="schur_jacobi")
    print("PRECONDREF 2-block grid lam=%g rel_tol=%g: block-Jacobi %d iterations (status %d), Schur-Jacobi %d (status %d)"
          % (lam, tol, bj["iterations"], bj["status"], sj["iterations"], sj["status"]))
    assert bj["status"] == 0 and sj["status"] == 0
    assert 2 * sj["iterations"] <= bj["iterations"], (sj["iterations"], bj["iterations"])


def test_both_preconditioners_reach_the_same_solution():
    P = _random(10)
    lam = 1e-3
    bj = PR.pcg_plain(P, lam, 400, 1e-15, kind="block_jacobi")
    sj = PR.pcg_plain(P, lam, 400, 1e-15, kind="schur_jacobi")
    assert bj["status"] == 0 and sj["status"] == 0
    xb, xs = bj["xs"][-1].astype(np.float64), sj["xs"][-1].astype(np.float64)
    assert np.linalg.norm(xb - xs) <= 1e-9 * np.linalg.norm(xb)
    same = R.pcg(P, lam, 5, 0.0, runs=0)
    mine = PR.pcg(P, lam, 5, 0.0, kind="block_jacobi", runs=0)       # the wrapper with _schurref's own preconditioner is _schurref.pcg
    assert all(np.array_equal(a, b) for a, b in zip(same["x"], mine["x"]))


# ---- 4. the boundary ----------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("c2b_problem_set_preconditioner", "c2b_problem_get_preconditioner", "c2b_problem_preconditioner_fallbacks",
               "c2b_schur_jacobi_rows", "c2b_schur_jacobi_rows_loss")


def test_library_exports_the_preconditioner_entries_under_a_new_abi_number():
    import __graft_entry__ as entry
    entry.build()
    from city2ba_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW_ENTRIES:
        assert hasattr(raw, n), "library does not export " + n
        assert n in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "city2ba_hip.h")).read()
    version = int(re.search(r"(?m)^#define C2B_ABI_VERSION (\d+)", header).group(1))
    raw.c2b_abi_version.restype = C.c_int
    assert raw.c2b_abi_version() == version == _lib.ABI_VERSION and version >= 8
    exp = open(os.path.join(ROOT, "include", "city2ba_hip_experimental.h")).read()
    assert re.search(r"(?m)^#define C2B_PRECOND_BLOCK_JACOBI 0$", exp) and re.search(r"(?m)^#define C2B_PRECOND_SCHUR_JACOBI 1$", exp)
    assert _lib.PRECOND_KINDS == {"block_jacobi": 0, "schur_jacobi": 1}
    # without a device the handle cannot exist; the argument checks that need none still answer
    assert raw.c2b_problem_set_preconditioner(None, 1) == _lib.ERR_INVALID_ARGUMENT
    assert raw.c2b_problem_preconditioner_fallbacks(None, None) == _lib.ERR_INVALID_ARGUMENT
