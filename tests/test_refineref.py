"""tests/_refineref.py without a GPU: on a one-point problem the per-point loop is _triangref.host_points_lm's loop iteration for
iteration (there the global and the per-point damping coincide), which ties the new reference to the existing one; the
float64 twin stays with the longdouble reference on the problems the GPU tests use; and the loop's statuses, tolerances,
priors and masks behave as DESIGN 4.16 words them."""
import numpy as np
import pytest

import _refineref as RR
import _triangref as T

LD = np.longdouble
LOSSES = [(None, 1.0), ("cauchy", 2e-3)]


def test_one_point_is_host_points_lm_iteration_for_iteration():
    P = RR.one_point_problem()
    n = 8
    costs, pts = T.host_points_lm(P, n)
    out = RR.refine(RR.of(P), P["pts"], rounds=n, lam=1e-4)
    got = [float(r["F"][0]) for r in out["rounds"]] + [float(out["F"][0])]
    # host_points_lm forms r and J in f64 from the oracle: its cost carries the rounding of a sum of 12 squares
    assert np.allclose(got, costs, rtol=1e-9, atol=0.0), (got, costs)
    assert costs[0] > 100 * costs[-1]                         # the loop had something to do
    for k, r in enumerate(out["rounds"]):                     # the decisions, where the cost moved by more than rounding
        if abs(costs[k] - costs[k + 1]) > 1e-9 * costs[k]:
            assert bool(r["accepted"][0])
    assert np.allclose(out["X"][0].astype(np.float64), pts[0], rtol=0, atol=1e-7)
    assert np.linalg.norm(pts[0] - P["true_pts"][0]) < 0.05


@pytest.mark.parametrize("loss,scale", LOSSES)
def test_the_twin_follows_the_reference_on_the_ragged_problem(loss, scale):
    P = RR.ragged_problem()
    Q = RR.of(P, loss=loss, loss_scale=scale)
    ref = RR.refine(Q, P["pts"], rounds=1)
    twin = RR.refine(Q, P["pts"], rounds=1, dtype=np.float64)
    edge = RR.borderline(ref["rounds"][0])
    tried = ref["rounds"][0]["tried"]
    assert edge.sum() <= 0.02 * tried.sum(), (int(edge.sum()), int(tried.sum()))
    same = ref["rounds"][0]["accepted"] == twin["rounds"][0]["accepted"]
    assert same[~edge].all()
    assert np.array_equal(ref["status"], twin["status"])
    tol, delta, ok = RR.step_tolerance(Q, P["pts"], 1e-4)
    acc = ref["moved"] & twin["moved"]
    err = np.linalg.norm((twin["X"].astype(LD) - ref["X"])[acc].astype(np.float64), axis=1)
    assert (err <= tol[acc]).all(), float((err / tol[acc]).max())
    assert ref["counts"]["unobserved"] == 38 and ref["counts"]["moved"] > 250


def test_never_worse_and_the_cost_falls_to_the_noise():
    P = RR.ragged_problem()
    Q = RR.of(P)
    out = RR.refine(Q, P["pts"], rounds=15)
    assert (out["F"] <= out["F0"])[np.isfinite(out["F0"].astype(np.float64))].all()
    assert float(out["F"].sum()) < 1e-2 * float(out["F0"].sum())
    F, B = Q.cost(out["X"])
    assert np.array_equal(F, out["F"])
    still = out["status"] != RR.MAX_ROUNDS
    assert np.array_equal(out["X"][still].astype(np.float64), P["pts"][still])


def test_statuses_masks_priors_and_tolerances():
    Pd, mask, (x0, xw) = RR.hand_placed()
    P, pts = RR.small_problem(), Pd["pts"]
    Q = RR.of(Pd, prior=(x0, xw), mask=mask)
    out = RR.refine(Q, pts, rounds=12)
    assert list(out["status"]) == [RR.MAX_ROUNDS, RR.CONSTANT, RR.FAILED, RR.MAX_ROUNDS, RR.MAX_ROUNDS, RR.MAX_ROUNDS, RR.UNOBSERVED, RR.MAX_ROUNDS]
    assert out["counts"] == dict(converged=0, max_rounds=5, unobserved=1, failed=1, constant=1, moved=5)
    X = out["X"].astype(np.float64)
    assert np.array_equal(X[[1, 6]], pts[[1, 6]]) and np.isnan(X[2]).all()
    assert np.allclose(X[7], x0[7], rtol=0, atol=1e-12)                     # the quadratic's minimum
    assert np.linalg.norm(X[[0, 3, 4, 5]] - P["true_pts"][[0, 3, 4, 5]], axis=1).max() < 1e-6
    zero = RR.refine(Q, pts, rounds=0)
    assert not zero["moved"].any() and zero["counts"]["max_rounds"] == 5
    # weights all 0 with NaN targets are no prior
    a = RR.refine(RR.of(Pd, prior=(np.full((8, 3), np.nan), np.zeros((8, 3))), mask=mask), pts, rounds=3)
    b = RR.refine(RR.of(Pd, mask=mask), pts, rounds=3)
    assert np.array_equal(a["X"][[0, 3, 4, 5]], b["X"][[0, 3, 4, 5]]) and np.array_equal(a["status"], b["status"])
    # the gradient and the parameter test end every point that runs
    free = RR.refine(Q, pts, rounds=12)
    for o in (RR.refine(Q, pts, rounds=12, gradient_tol=1e-6), RR.refine(Q, pts, rounds=12, parameter_tol=1e-6)):
        assert (o["status"][[0, 3, 4, 5, 7]] == RR.CONVERGED).all() and o["counts"]["converged"] == 5
        assert np.allclose(o["X"][[0, 3, 4, 5, 7]].astype(np.float64), free["X"][[0, 3, 4, 5, 7]].astype(np.float64), rtol=0, atol=1e-4)


def test_the_function_test_ends_the_points_whose_cost_has_a_floor():
    """noisy pixels leave a point seen three times or more a cost > 0, which the function test meets; a point seen once or
    twice fits its pixels exactly, its cost falls by orders of magnitude per round to 0, and the relative test never fires"""
    P = RR.ragged_problem()
    Q = RR.of(P)
    out = RR.refine(Q, P["pts"], rounds=20, function_tol=1e-6)
    many = Q.count >= 5
    assert (out["status"][many] == RR.CONVERGED).all() and many.sum() > 140
    free = RR.refine(Q, P["pts"], rounds=20)
    assert (free["status"][Q.count > 0] == RR.MAX_ROUNDS).all()
    assert ((out["F"] - free["F"])[many] <= 1e-5 * free["F"][many]).all()


def test_a_point_seen_once_is_carried_by_the_damping():
    P = RR.ragged_problem()
    once = np.flatnonzero(np.bincount(P["pt_idx"].astype(np.int64), minlength=300) == 1)
    assert len(once) > 30
    Q = RR.of(P)
    cur = Q.walk(P["pts"])
    ev = np.linalg.eigvalsh(cur["V"][once].astype(np.float64))
    assert (ev[:, 0] <= 1e-9 * ev[:, 2]).all()                # rank 2: the depth is not observed
    out = RR.refine(Q, P["pts"], rounds=10)
    assert np.isfinite(out["X"][once].astype(np.float64)).all() and (out["F"][once] < 1e-6 * out["F0"][once]).all()
