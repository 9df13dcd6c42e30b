"""tests/_explicitref.py held to what is already trusted, without a GPU: its blocks, assembled dense, are
_schurref.Problem.dense_S; its diagonal is _precondref.schur_diag_blocks; its pattern is _covisref.graph at threshold 1; its
product is the dense product; its perturbed reruns move the blocks by a few eps of their scale and no more; and its PCG
follows the implicit reference's on a problem both solve."""
import numpy as np
import pytest

import _covisref as CR
import _explicitref as X
import _precondref as PR
import _schurref as R
import _solvecheck as SC
from _problems import dome_problem, random_problem

_cache = {}


def _problem(name, dtype=R.LD):
    key = (name, dtype)
    if key not in _cache:
        if name == "random":                                  # every point seen once: no edge at all
            import oracle as O
            Q = random_problem(30, 300, 8, seed=11, noise=1e-3, empty_every=7)
            r, Jc, Jp = O.residual_jacobian_bal(Q["bal9"], Q["pts"], Q["row_ptr"], Q["pt_idx"], Q["uv"])
            _cache[key] = SC.linearisation(r, Jc, Jp, Q["row_ptr"], Q["pt_idx"], len(Q["bal9"]), len(Q["pts"]), dtype)
        else:
            _cache[key] = SC.oracle_problem(dome_problem(dup=name == "dome dup"), dtype=dtype)
    return _cache[key]


NAMES = ["dome dup", "dome nodup", "random"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_blocks_assembled_dense_are_dense_S(name, lam):
    """dense_S is an f64 evaluation of the same definition (adjugate inverse, two 9x3 products and a sum per term): a few
    roundings per term, so it is held to 16 eps of the reference's own absolute-value scale, block by block"""
    P = _problem(name)
    ref = X.blocks(P, lam)
    S, want = X.dense(ref, P.n_cam), P.dense_S(lam)
    scale = X.dense(dict(ref, D=ref["SD"], E=ref["SE"]), P.n_cam)
    assert not want[scale == 0].any()                         # nothing outside the pattern
    worst = 0.0
    for c in range(P.n_cam):
        for q in range(P.n_cam):
            blk = (slice(9 * c, 9 * c + 9), slice(9 * q, 9 * q + 9))
            s = np.linalg.norm(scale[blk])
            if s:
                worst = max(worst, np.linalg.norm(S[blk] - want[blk]) / (16 * R.EPS * s))
    print("EXPLICITREF dense %s lam=%g: worst |err| / (16 eps scale) %.3g" % (name, lam, worst))
    assert worst <= 1.0
    assert np.array_equal(S, S.T) or np.allclose(S, S.T, rtol=0, atol=16 * R.EPS * np.abs(scale).max())


@pytest.mark.parametrize("name", NAMES)
def test_diagonal_is_schur_diag_blocks_and_pattern_is_the_graph(name):
    P = _problem(name)
    lam = 1e-2
    ref = X.blocks(P, lam)
    D, SD = PR.schur_diag_blocks(P, lam)
    err = np.linalg.norm((ref["D"] - D).astype(np.float64), axis=(1, 2))
    assert (err <= 64 * float(np.finfo(R.LD).eps) * np.linalg.norm(SD.astype(np.float64), axis=(1, 2))).all(), err.max()
    # (its scale sums |Jc|^T |Jp| where schur_diag_blocks takes |Jc^T Jp|: never smaller)
    assert (ref["SD"].astype(np.float64) >= SD.astype(np.float64) * (1 - 1e-12)).all()
    nbr_ptr, nbr, _ = CR.graph(X.row_ptr_of(P), P.pt, 1)
    assert ref["nbr_ptr"].tobytes() == nbr_ptr.tobytes() and ref["nbr"].tobytes() == nbr.tobytes()
    assert ref["nbr_ptr"].dtype == np.uint64 and ref["nbr"].dtype == np.uint32
    if name == "random":
        assert len(nbr) == 0
    else:
        assert PR.has_duplicate_pairs(P) == (name == "dome dup") and len(nbr) == 2 * 3160
        # (c', c) is the transpose of (c, c')
        eid, row = X._edge_ids(ref["nbr_ptr"], ref["nbr"], P.n_cam)
        back = eid[ref["nbr"].astype(np.int64), row]
        assert (back >= 0).all()
        gap = np.abs(ref["E"] - ref["E"][back].transpose(0, 2, 1)).astype(np.float64)
        assert (gap <= 64 * float(np.finfo(R.LD).eps) * ref["SE"].astype(np.float64)).all()


def test_duplicated_pairs_are_in_the_diagonal():
    P = _problem("dome dup")
    lam = 1e-2
    ref = X.blocks(P, lam)
    M, _ = PR.blocks(P, lam)
    gap = np.linalg.norm((ref["D"] - M).astype(np.float64), axis=(1, 2))
    bound = X.blocks_bound(P, lam, runs=2)["bound_D"]
    assert (gap > bound).any()                                # S's diagonal is not M where a pair repeats ...
    Q = _problem("dome nodup")
    refq, Mq = X.blocks_bound(Q, lam, runs=2), PR.blocks_bound(Q, lam, runs=2)
    gapq = np.linalg.norm((refq["D"] - Mq[0]).astype(np.float64), axis=(1, 2))
    assert (gapq <= refq["bound_D"] + Mq[1]).all()            # ... and is M where none does


def test_perturbed_reruns_give_bounds_of_a_few_eps_of_the_scale():
    P = _problem("dome dup")
    for lam in (1e-4, 1.0):
        ref = X.blocks_bound(P, lam, runs=8)
        for b, s in ((ref["bound_D"], ref["SD"]), (ref["bound_E"], ref["SE"])):
            n = np.linalg.norm(s.astype(np.float64), axis=(1, 2))
            assert (b >= 1e-13 * n).all() and (b[n > 0] > 0).all()
            assert (b <= 1e4 * R.EPS * n).all(), float((b / n).max())      # never a bound that holds nothing


def test_product_is_the_dense_product_and_the_pcg_follows_the_implicit_reference():
    P = _problem("dome nodup")
    lam = 1.0
    ref = X.blocks(P, lam)
    x = np.random.default_rng(5).normal(size=(P.n_cam, 9)).astype(R.LD)
    y, s = X.spmv(ref["nbr_ptr"], ref["nbr"], ref["D"], ref["E"], x)
    want = X.dense(ref, P.n_cam) @ x.astype(np.float64).reshape(-1)
    assert np.linalg.norm(y.astype(np.float64).reshape(-1) - want) <= 1e-13 * np.linalg.norm(s.astype(np.float64))
    yi, si = P.S_times(lam, x)
    assert np.linalg.norm((y - yi).astype(np.float64)) <= 1e-15 * np.linalg.norm((s + si).astype(np.float64))
    ks = 6
    a = X.pcg(P, lam, ks, 0.0, kind="block_jacobi", runs=2)
    b = PR.pcg(P, lam, ks, 0.0, kind="block_jacobi", runs=2)
    assert a["iterations"] == b["iterations"] == ks
    for k in range(ks + 1):
        gap = float(np.linalg.norm((a["x"][k] - b["x"][k]).astype(np.float64)))
        assert gap <= a["bound"]["x"][k] + b["bound"]["x"][k], (k, gap)
