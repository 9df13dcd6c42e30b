"""Resection-intersection alternation (solve.alternate): refine_cameras and refine_points in turn on the device.
Cameras and points both start displaced and the gauge is fixed by constant cameras.  The cost history does not rise beyond the
cost's summation bound, and the first sweep is, bit for bit, the two calls made by hand."""
import numpy as np
import pytest

import _refinecamref as RC
from test_gpu_schur_step import _bits, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def _start(loss):
    """the noisy dome with the cameras 0.02 rad / 0.05 and the points 0.03 from the truth; cameras 0 .. 2 constant (the gauge)"""
    import city2ba_amd as c2b
    from city2ba_amd import solve as S
    P = RC.dome(1e-3)
    g = np.random.default_rng(4).normal(size=P["pts"].shape)
    pts = P["pts"] + 0.03 * g / np.linalg.norm(g, axis=1)[:, None]
    ba = c2b.BAProblem.from_bal(P["bal9"], pts, P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    mask = np.zeros(len(P["bal9"]), dtype=np.uint16)
    mask[:3] = S.ALL
    ba.set_constant(cameras=mask)
    if loss:
        ba.set_loss(loss, 5e-3)
    return P, ba, mask


@pytest.mark.parametrize("loss", [None, "cauchy"], ids=["squared", "cauchy"])
def test_the_cost_history_does_not_rise_and_the_first_sweep_is_the_two_calls(env, loss):
    from city2ba_amd import solve as S
    P, ba, mask = _start(loss)
    b0 = ba.cameras_bal()
    out = S.alternate(ba, sweeps=6, camera_rounds=3, point_rounds=3)
    costs = np.asarray(out["costs"])
    n_obs = len(P["pt_idx"])
    # a sum of n_obs non-negative terms in any f64 order: within n_obs 2^-52 of its exact value, at either end of a sweep
    slack = 2.0 * n_obs * EPS * costs[:-1]
    print("ALTERNATE %s: costs %s; cameras %s; points %s" % (loss, ["%.6g" % c for c in costs], out["cameras"], out["points"]))
    assert out["sweeps"] == 6 and len(costs) == 7
    assert (np.diff(costs) <= slack).all(), np.diff(costs)
    assert costs[-1] < costs[0]
    assert _bits(ba.cameras_bal()[:3], b0[:3]) and out["cameras"]["constant"] == 3
    _, bb, _ = _start(loss)
    one = S.alternate(bb, sweeps=1, camera_rounds=3, point_rounds=3)
    _, bc, _ = _start(loss)
    cams = bc.refine_cameras(rounds=3)
    pts = bc.refine_points(rounds=3)
    assert one["cameras"] == cams and one["points"] == pts and one["costs"][1] == costs[1]
    assert _bits(bb.cameras_bal(), bc.cameras_bal()) and _bits(bb.points(), bc.points())
    for h in (ba, bb, bc):
        h.close()


def test_the_function_tolerance_stops_early(env):
    from city2ba_amd import solve as S
    _, ba, _ = _start(None)
    out = S.alternate(ba, sweeps=40, camera_rounds=3, point_rounds=3, function_tol=0.2)
    c = out["costs"]
    assert 1 <= out["sweeps"] < 40 and len(c) == out["sweeps"] + 1
    assert c[-2] - c[-1] <= 0.2 * c[-2] and all(c[k] - c[k + 1] > 0.2 * c[k] for k in range(len(c) - 2))
    ba.close()
