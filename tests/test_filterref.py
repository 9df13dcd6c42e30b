"""The outlier filter's host reference (tests/_filterref.py) decides every case the GPU tests run in double: on each
problem the double mask and its longdouble twin agree at every threshold used, because every threshold sits in the middle
of a relative gap of at least 1e-9 between two adjacent residuals and every |q.z| is far from zero.  No observation is left
out of the exact comparison.  Conditions, checked without a GPU."""
import numpy as np
import pytest

import _filterref as F

EPS = float(np.finfo(np.float64).eps)


def _check(P, thresholds, in_front):
    args = (P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])
    r2, qz = F.residuals(*args)
    r2l, qzl, dist, mag = F.residuals_ld(*args)
    n = len(r2)
    # the tail's five operations lose at most 3 eps of r2; q.z (three products, three sums) at most 4 eps of its terms' magnitudes
    assert np.all(np.abs(r2l - r2.astype(F.LD)) <= 3 * EPS * r2l)
    assert np.all(np.abs(qzl - qz.astype(F.LD)) <= 4 * EPS * mag)
    assert np.all(np.abs(qzl) > 1e-9 * dist), "a point sits on its camera's plane: the in-front test is not decidable"
    assert np.array_equal(qz < 0.0, qzl < 0.0)
    left_out = 0
    for t in thresholds:
        m2 = F.max_err2(t)
        if np.isfinite(m2) and m2 > 0.0:
            s = np.sort(r2)
            k = int(np.searchsorted(s, m2))
            assert 0 < k < n and s[k - 1] < m2 < s[k] and s[k] - s[k - 1] >= F.GAP * s[k], (t, k)
            assert min(m2 - s[k - 1], s[k] - m2) >= 0.25 * F.GAP * s[k]            # the square of the root stays mid-gap
            left_out += int(np.sum(np.abs(r2l - F.LD(m2)) <= 8 * EPS * F.LD(m2)))
        for front in ((False, True) if in_front else (False,)):
            keep = F.keep_mask(r2, qz, t, front)
            with np.errstate(invalid="ignore"):
                twin = r2l <= F.LD(m2)
                if front:
                    twin = twin & (qzl < 0)
            assert np.array_equal(keep, twin), (t, front)
    assert left_out == 0
    return r2, qz


@pytest.mark.parametrize("dup,state,behind", F.DOME_CASES)
def test_dome_thresholds_are_decided_in_double(dup, state, behind):
    P = F.dome_case(dup, state, behind)
    lo, hi = P["thresholds"]
    assert lo < hi
    r2, qz = _check(P, P["thresholds"], in_front=True)
    n = len(r2)
    kept = [int(F.keep_mask(r2, qz, t).sum()) for t in P["thresholds"]]
    assert abs(kept[0] - 0.5 * n) <= 2 and abs(kept[1] - 0.9 * n) <= 2, (kept, n)   # the percentiles they were placed at
    if behind:
        at = P["moved"]
        assert len(at) == F.BEHIND and np.all(r2[at] == 0.0) and np.all(qz[at] > 1.0)
        assert int(F.keep_mask(r2, qz, 0.0).sum()) == F.BEHIND   # ... and they alone sit exactly on the bound 0
        for t in P["thresholds"]:                                # only the in-front test removes them
            assert np.all(F.keep_mask(r2, qz, t)[at]) and not np.any(F.keep_mask(r2, qz, t, True)[at])
    else:
        assert np.all(qz < 0.0)


@pytest.mark.parametrize("n_obs", F.COUNT_EDGES)
def test_count_edge_thresholds_are_decided_in_double(n_obs):
    P = F.count_case(n_obs)
    assert int(P["row_ptr"][-1]) == n_obs == len(P["pt_idx"])
    assert np.any(np.diff(P["row_ptr"].astype(np.int64)) == 0)                     # empty cameras
    ts = [0.0, float("inf")] + ([P["threshold"]] if P["threshold"] is not None else [])
    r2, qz = _check(P, ts, in_front=False)
    assert np.all(r2 > 0.0) and np.all(np.isfinite(r2))                            # 0 keeps none, inf keeps all
    assert not F.keep_mask(r2, qz, 0.0).any() and F.keep_mask(r2, qz, float("inf")).all()


def test_filtered_lists_keep_the_order_inside_every_row():
    P = F.dome_case(True, False)
    keep, rows, pi, uv, removed = F.reference(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], P["thresholds"][0])
    assert removed == int((~keep).sum()) > 0 and int(rows[-1]) == len(pi) == len(uv) == int(keep.sum())
    old = P["row_ptr"].astype(np.int64)
    for c in range(len(old) - 1):
        k = keep[old[c]:old[c + 1]]
        assert np.array_equal(pi[int(rows[c]):int(rows[c + 1])], P["pt_idx"][old[c]:old[c + 1]][k])
    bad = P["uv"].copy()
    bad[3] = np.nan
    bad[7, 0] = np.inf
    big = 1e3                                                    # finite, above every finite residual here
    keep2 = F.reference(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], bad, big)[0]
    assert not keep2[3] and not keep2[7] and keep2.sum() == len(keep2) - 2
    keep3 = F.reference(P["cams15"], P["pts"], P["row_ptr"], P["pt_idx"], bad, float("inf"))[0]
    assert not keep3[3] and keep3[7] and keep3.sum() == len(keep3) - 1          # inf <= inf: only the NaN goes
