"""tests/_problems.py's dome_problem and the longdouble references on it, on the CPU with the oracle's Jacobian: what
tests/test_gpu_coupled.py relies on.  The row lengths that are chosen are all there, cameras do not come in fours, one
point's row is longer than a wave, unobserved points and points seen once exist, (camera, point) pairs repeat (and do
not with dup=False), every observed point is in front of its camera; both reference PCGs run every compared iterate
without a breakdown; and at each compared iterate the reference's own bound on x and dp is at most 1e-6 of the
iterate's norm (_solvecheck.DOME_CAP): a cap, so that the bound the device is held to cannot grow loose enough to hide a
wrong kernel."""
import numpy as np
import pytest

import _precondref as PR
import _schurref as R
import _solvecheck as SC
from _problems import (DOME_CROWDED, DOME_LENGTHS, DOME_N_CAM, DOME_N_PTS, DOME_SINGLES, DOME_UNOBSERVED, dome_problem)

LD = R.LD
ELD = float(np.finfo(LD).eps)


@pytest.fixture(scope="module")
def dome():
    import __graft_entry__ as entry
    entry.build()                                                # the oracle's library
    return {(dup, state): dome_problem(dup=dup, state=state) for dup in (True, False) for state in (False, True)}


def test_shape_of_the_lists(dome):
    for (dup, state), P in dome.items():
        kc = np.diff(P["row_ptr"].astype(np.int64))
        pt = P["pt_idx"].astype(np.int64)
        kp = np.bincount(pt, minlength=DOME_N_PTS)
        assert len(kc) == DOME_N_CAM == 81 and DOME_N_CAM % 4 == 1 and len(P["pts"]) == DOME_N_PTS == 400
        assert set(DOME_LENGTHS) <= set(kc.tolist()) and np.array_equal(kc, P["lengths"])
        assert 2000 <= len(pt) <= 3500, len(pt)
        # a long row, an empty one and short ones share a wave of four cameras somewhere
        waves = [set(kc[q:q + 4].tolist()) for q in range(0, DOME_N_CAM, 4)]
        assert any(max(w) >= 127 and min(w) <= 5 for w in waves), waves
        assert kp[DOME_CROWDED] == kp.max() > 64 and kp[DOME_CROWDED] >= (kc > 0).sum()
        assert not kp[-DOME_UNOBSERVED:].any() and kp[:-DOME_UNOBSERVED].all()
        assert (kp == 1).sum() >= DOME_SINGLES >= 36, (kp == 1).sum()
        Q = SC.oracle_problem(P)
        assert PR.has_duplicate_pairs(Q) == dup
        if dup:                                                  # the repeats are not adjacent, the crowded point's among them
            cam = SC.cam_of(P["row_ptr"])
            key = cam * DOME_N_PTS + pt
            o = np.argsort(key, kind="stable")
            same = np.flatnonzero(key[o][1:] == key[o][:-1])
            assert len(same) >= 8 and (o[same + 1] - o[same] >= 2).all()
            assert (pt[o[same]] == DOME_CROWDED).any() and (pt[o[same]] != DOME_CROWDED).any()
            assert kp[DOME_CROWDED] > (kc > 0).sum()
        # mixed k2 in a wave of four cameras and in one point's walk
        k2 = P["bal9"][:, 8]
        assert (k2[::5] == 0).all() and (np.delete(k2, np.arange(0, DOME_N_CAM, 5)) != 0).all()
        assert P["bal"] == (not state)
        w = np.linalg.norm(P["bal9"][:, :3], axis=1)
        assert w.min() > 0.1 and w.max() < 2 * np.pi and (w > np.pi).any() and (w < 1.5).any()      # general rotations, large angles


def test_every_observed_point_is_in_front_of_its_camera(dome):
    P = dome[(True, False)]
    cam, pt = SC.cam_of(P["row_ptr"]), P["pt_idx"].astype(np.int64)
    Rm = P["cams15"][cam, :9].reshape(-1, 3, 3).transpose(0, 2, 1)       # column-major R: q = R X + t
    q = np.einsum("nij,nj->ni", Rm, P["pts"][pt]) + P["cams15"][cam, 9:12]
    assert q[:, 2].max() <= -1.0, q[:, 2].max()
    assert np.abs(P["uv"]).max() < 0.6
    r = SC.oracle_problem(P).r
    assert 1e-4 < np.abs(r).max() < 1e-2                        # moved from the observations: the gradient is not zero


@pytest.mark.parametrize("lam", [1e-4, 1.0])
@pytest.mark.parametrize("kind", ["block_jacobi", "schur_jacobi"])
def test_reference_pcg_runs_and_its_bounds_stay_under_the_cap(dome, kind, lam):
    """(The oracle's Jacobian has the same columns in both modes; the device's state mode has its own, and
    test_gpu_coupled.py asserts the cap again on every reference it builds from the device's Jacobian.)"""
    Q = SC.oracle_problem(dome[(True, False)], dtype=LD)
    ks = SC.DOME_KS[(kind, lam)]
    assert set((0, 1, 2)) <= set(ks) and sum(k > 2 for k in ks) >= 3
    ref = PR.pcg(Q, lam, max(ks), 0.0, kind=kind, runs=8)
    assert ref["status"] == 1 and ref["iterations"] == max(ks) and len(ref["x"]) == max(ks) + 1
    cap = SC.cap_excess(ref, ks)
    print("COUPLED cap %s lam=%g: worst bound / (1e-6 |iterate|) %.3g" % (kind, lam, cap))
    assert cap <= 1.0, (kind, lam, cap)
    if kind == "schur_jacobi":
        piv = PR.pivots(PR.blocks(Q, lam)[0])
        assert np.isfinite(piv.astype(np.float64)).all() and (piv > 0).all(), float(piv.min())


@pytest.mark.parametrize("variant", ["cauchy", "mask block_jacobi", "mask schur_jacobi", "cauchy mask schur_jacobi"])
def test_reference_bounds_of_the_variants_stay_under_the_cap(dome, variant):
    """the loss and mask cases of test_gpu_coupled.py, at their lam = 1e-2 and iterates"""
    P = dome[(True, False)]
    uv = loss = mask = None
    if "cauchy" in variant:
        uv, pick = SC.dome_scaled_observations(P)
        assert 0.05 < pick.mean() < 0.15
        loss = ("cauchy", SC.cauchy_scale(SC.oracle_problem(P, uv=uv).r))
    if "mask" in variant:
        mask = SC.dome_mask(P)
    kind = "schur_jacobi" if "schur_jacobi" in variant else "block_jacobi"
    Q = SC.oracle_problem(P, dtype=LD, uv=uv, loss=loss, mask=mask)
    ks = SC.DOME_KS_SHORT
    ref = PR.pcg(Q, 1e-2, max(ks), 0.0, kind=kind, runs=8)
    assert ref["status"] == 1 and ref["iterations"] == max(ks)
    cap = SC.cap_excess(ref, ks)
    print("COUPLED cap %s: worst bound / (1e-6 |iterate|) %.3g" % (variant, cap))
    assert cap <= 1.0, (variant, cap)


@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_schur_jacobi_blocks_are_the_diagonal_blocks_of_s_without_duplicates_only(dome, lam):
    """test_precondref.py's criterion: both sides are sums of longdouble products whose absolute values add up to SM and
    SD, 512 eps of longdouble per entry.  With duplicates the cameras that see a point twice differ by the cross terms,
    which no rounding explains; the others still agree."""
    def excess(P):
        M, SM = PR.blocks(P, lam)
        D, SD = PR.schur_diag_blocks(P, lam)
        b = 512 * ELD * (SM + SD).astype(np.float64)
        e = np.abs(M - D).astype(np.float64)
        with np.errstate(all="ignore"):
            return np.where(b > 0, e / b, np.where(e == 0, 0.0, np.inf)).max(axis=(1, 2))

    assert excess(SC.oracle_problem(dome[(False, False)], dtype=LD)).max() <= 1.0
    Q = SC.oracle_problem(dome[(True, False)], dtype=LD)
    key = Q.cam * Q.n_pts + Q.pt
    u, n = np.unique(key, return_counts=True)
    twice = np.zeros(Q.n_cam, dtype=bool)
    twice[u[n > 1] // Q.n_pts] = True
    ex = excess(Q)
    assert twice.sum() >= 8 and ex[~twice].max() <= 1.0
    if lam == 1.0:                                               # at small lam |V_l^-1| ~ 1 / lam of the points seen once swamps the scale
        assert ex[twice].min() > 1e3, ex[twice].min()


def test_host_lm_reaches_the_noise_floor(dome):
    """what test_gpu_coupled.py's LM run is compared with: the dense-solve loop falls on every accepted step and ends
    below the error of the state the observations were made from (it fits the noise)"""
    P = dome[(True, True)]
    e = SC.host_lm(P, 10)
    floor = dict(P, bal9=P["true_bal9"], pts=P["true_pts"], bal=True)
    e_floor = float(np.sum(SC.oracle_problem(floor).r ** 2))
    print("COUPLED host LM: %s; noise floor %.6e" % (["%.6e" % v for v in e], e_floor))
    assert all(b <= a for a, b in zip(e, e[1:])) and e[-1] < e[0]
    assert e[-1] <= e_floor
