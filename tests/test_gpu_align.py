"""The similarity alignment on the device against the long-double reference of tests/_alignref.py: the two moment passes
at the edges of their launch shape, the fit end to end, the rotation errors, the summaries, trimming, transform, determinism, the
refusals, the leak test and one use -- a free-gauge solve compared against the truth."""

import functools

import numpy as np
import pytest

import _alignref as A
from _problems import NOISE_VARIANTS, dome_problem, grid_problem, noise_problem

pytestmark = pytest.mark.gpu
U = A.U


@pytest.fixture(scope="module")
def c2b():
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd
    assert city2ba_amd.device_count() > 0
    return city2ba_amd


@pytest.fixture(scope="module")
def dev(c2b):
    import torch
    from city2ba_amd import device as D
    from city2ba_amd import _lib as L
    return dict(torch=torch, D=D, L=L, ws=D.workspace(0, "cuda:0"))


def _rows4(dev, a):
    t = dev["torch"].zeros((len(a), 4), dtype=dev["torch"].float64, device="cuda:0")
    if len(a):
        t[:, :3] = dev["torch"].from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return t


# ---- the moment passes --------------------------------------------------------------------------------------------------------------
_clouds = {}


def _cloud(variant, n):
    """n correspondences of a variant: the first n // 2 play the cameras' part, the rest the points'; x the cloud, y its known similarity"""
    if variant not in _clouds:
        from city2ba_amd import _lib as L
        block, grid, _ = L.align_launch_shape()
        x = noise_problem(0, block * grid + 1, seed=41 + NOISE_VARIANTS.index(variant), variant=variant)["pts"]
        _clouds[variant] = (x, A.move(x))
    x, y = _clouds[variant]
    return x[:n], y[:n]


def _counts():
    from city2ba_amd import _lib as L
    block, grid, _ = L.align_launch_shape()                   # the numbers are the launcher's: one full grid = block * grid entities
    return (3, 4, 63, 64, 65, 255, 256, 257, block * grid - 1, block * grid, block * grid + 1)


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("variant", NOISE_VARIANTS)
def test_means_and_centred_moments_within_the_summation_bound(dev, variant, masked):
    """means and the eleven centred sums against the long-double reference within (n + 8) u sum |term|, the classical bound for any
    summation order -- on `offset` (a cloud at 1e6 with a spread of 1e-3) relative to the CENTRED terms, which a raw-moment form
    misses by many orders of magnitude"""
    D, L, ws, torch = dev["D"], dev["L"], dev["ws"], dev["torch"]
    worst = 0.0
    for n in _counts():
        x, y = _cloud(variant, n)
        nc = n // 2
        on = np.ones(n, dtype=bool)
        if masked:
            on[::3] = False                                   # every third entity off
        tx, ty = _rows4(dev, x), _rows4(dev, y)
        m8 = torch.from_numpy(on.astype(np.uint8)).to("cuda:0")
        kw = dict(x_cam=tx[:nc], y_cam=ty[:nc], x_pts=tx[nc:], y_pts=ty[nc:])
        if masked:
            kw.update(use_cam=m8[:nc].contiguous(), use_pt=m8[nc:].contiguous())
        if nc == 0:
            kw.update(x_cam=None, y_cam=None, use_cam=None)
        means = D.align_means_rows(ws, **kw)
        mom = D.align_moments_rows(ws, means, **kw)
        got = L.align_finish_moments(means.cpu().numpy(), mom.cpu().numpy())
        ref = A.moments(x, y, on)
        k = ref["n"]
        b = (k + 8) * U
        assert got["n"] == k, (variant, n)
        sums = means.cpu().numpy()
        assert np.all(np.abs(sums[1:4] - ref["mean_x"] * k) <= b * ref["abs_mean_x"]) and np.all(np.abs(sums[4:7] - ref["mean_y"] * k) <= b * ref["abs_mean_y"])
        assert np.all(np.abs(got["mean_x"] - ref["mean_x"]) <= b * ref["abs_mean_x"] / k) and np.all(np.abs(got["mean_y"] - ref["mean_y"]) <= b * ref["abs_mean_y"] / k)
        diff = np.concatenate([[abs(got["var_x"] * k - ref["sxx"]), abs(got["var_y"] * k - ref["syy"])], np.abs(got["cov"] * k - ref["sxy"]).ravel()]).astype(np.float64)
        bound = (b * np.concatenate([[ref["abs_sxx"], ref["abs_syy"]], ref["abs_sxy"].ravel()])).astype(np.float64)
        assert np.all(diff <= bound), (variant, n, masked, diff / bound)       # (a zero bound -- the planar cloud's flat axis -- asks for an exact zero)
        worst = max(worst, float((diff[bound > 0] / bound[bound > 0]).max()))
    print("%s%s: worst |device - reference| / bound over the counts %.3g" % (variant, " masked" if masked else "", worst))


# ---- the fit end to end --------------------------------------------------------------------------------------------------------------
def _upload(c2b, cams15, pts, G=None, bal9=None):
    if G is None:
        rp, pi, uv = np.zeros(len(cams15 if bal9 is None else bal9) + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2))
    else:
        rp, pi, uv = G["row_ptr"], G["pt_idx"], G["uv"]
    if bal9 is not None:
        return c2b.BAProblem.from_bal(bal9, pts, rp, pi, uv)
    return c2b.BAProblem.from_visibility(cams15, pts, rp, pi, uv)


@functools.lru_cache(maxsize=None)
def _truths():
    """the true dome and the grid, built once: name -> (cams15, pts, the problem's dict); read, never written"""
    import oracle as O
    d = dome_problem(seed=0)
    g = grid_problem()
    return {"dome": (O.camera_from_bal(d["true_bal9"]), d["true_pts"], d), "grid": (g["cams15"], g["pts"], g)}


def _d_sigma(ref):
    k = ref["n"]
    cov = (ref["sxy"] / k).astype(np.float64)
    return float(np.sqrt((((k + 8) * U * ref["abs_sxy"] / k) ** 2).sum())) + 64 * U * float(np.sqrt((cov * cov).sum()))


@pytest.mark.parametrize("on", ("cameras", "points", "both"))
@pytest.mark.parametrize("name", ("dome", "grid"))
def test_fit_recovers_the_similarity_within_the_polar_bound(c2b, name, on):
    """the estimate = the truth moved by the known similarity, aligned back onto the truth: (s, R, t) within the polar-factor bound with
    |dSigma| from the moment bound, the per-entity errors within 8u (s |x| + |t| + |y|) of the reference's, scale=False gives s == 1.0
    exactly, and two calls give the same bits"""
    cams, pts, _ = _truths()[name]
    mc, mp = A.apply(cams, pts, A.S0, A.R0, A.T0)
    est, ref = _upload(c2b, mc, mp), _upload(c2b, cams, pts)
    xc, yc = est._camera_centers(), ref._camera_centers()       # the centre tables the passes read
    sel = {"cameras": (xc, yc), "points": (mp, pts), "both": (np.concatenate([xc, mp]), np.concatenate([yc, pts]))}[on]
    got = est.align(ref, on=on, return_errors=True, return_inliers=True)
    again = est.align(ref, on=on, return_errors=True, return_inliers=True)
    for k in ("scale", "rotation", "translation", "camera_errors", "camera_rotation_errors", "point_errors", "camera_inliers", "point_inliers"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(again[k])), k
    assert got["cameras"] == again["cameras"] and got["points"] == again["points"] and got["status"] == "ok" and got["rounds"] == 0
    st, s, R, t, sig, eps = A.fit(*sel)
    m = A.moments(*sel)
    dR, ds, dt = A.fit_bounds(m, sig, eps, s, _d_sigma(m), (m["n"] + 8) * U)
    print("%s/%s: |dR|_F %.3g (bound %.3g)  ds %.3g (%.3g)  |dt| %.3g (%.3g)" % (name, on, np.sqrt(((got["rotation"] - R) ** 2).sum()), dR,
                                                                                abs(got["scale"] - s), ds, np.sqrt(((got["translation"] - t) ** 2).sum()), dt))
    assert st == A.OK and np.sqrt(((got["rotation"] - R) ** 2).sum()) <= dR and abs(got["scale"] - s) <= ds
    assert np.sqrt(((got["translation"] - t) ** 2).sum()) <= dt
    T = (got["scale"], got["rotation"], got["translation"])
    for key, x, y in (("camera_errors", xc, yc), ("point_errors", mp, pts)):
        e = A.errors(x, y, *T)
        assert np.all(np.abs(got[key] - e) <= A.error_bound(x, y, T[0], T[2])), key
        S = A.summary(e)
        G = got["cameras" if key == "camera_errors" else "points"]
        k = S["n"]
        assert G["n"] == k and G["argmax"] == int(np.argmax(got[key])) and G["max"] == got[key].max()
        assert abs(G["mean"] * k - S["sum"]) <= (k + 8) * U * S["sum"] + k * A.error_bound(x, y, T[0], T[2]).max()
    th, q = A.rotation_errors(mc, cams, got["rotation"])
    assert np.all(np.abs(got["camera_rotation_errors"] - th) <= A.rotation_error_bound(q))
    unit = est.align(ref, on=on, scale=False)
    assert unit["scale"] == 1.0 and unit["status"] == "ok"


def test_rotation_errors_keep_small_angles(dev):
    """cameras turned by 0, 1e-9, 1e-4, 1, pi - 1e-6 and pi about random axes: theta within the first-order bound of the reference's, the
    1e-9 case to a relative 1e-6 -- which acos of the trace cannot deliver"""
    D, L, ws, torch = dev["D"], dev["L"], dev["ws"], dev["torch"]
    P = noise_problem(6, 0, seed=23)["cams15"]
    rng = np.random.default_rng(5)
    angles = np.array([0.0, 1e-9, 1e-4, 1.0, np.pi - 1e-6, np.pi])
    turned = P.copy()
    for k, a in enumerate(angles):
        Rc = P[k, :9].reshape(3, 3).T.astype(A.LD)
        turned[k, :9] = (A.rotation(rng.normal(size=3), a).astype(A.LD) @ Rc).T.reshape(9).astype(np.float64)
    for R in (np.eye(3), A.R0):
        ref15 = P.copy()
        ref15[:, :9] = ((P[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1).astype(A.LD) @ R.astype(A.LD).T).transpose(0, 2, 1)).reshape(-1, 9).astype(np.float64)
        err = torch.zeros(6, dtype=torch.float64, device="cuda:0")
        out = D.align_rotation_errors_rows(ws, torch.from_numpy(turned).to("cuda:0"), torch.from_numpy(ref15).to("cuda:0"), L.similarity(1.0, R, [0, 0, 0]), err=err)
        th, q = A.rotation_errors(turned, ref15, R)
        got = err.cpu().numpy()
        assert np.all(np.abs(got - th) <= A.rotation_error_bound(q)), (got - th.astype(np.float64), A.rotation_error_bound(q))
        assert int(out[0].item()) == 6 and out[3].item() == got.max() and int(out[4].item()) == int(np.argmax(got))
    th, _ = A.rotation_errors(turned, P, np.eye(3))             # against the cameras themselves: the angle of the f64 inputs is the one applied
    err = torch.zeros(6, dtype=torch.float64, device="cuda:0")
    D.align_rotation_errors_rows(ws, torch.from_numpy(turned).to("cuda:0"), torch.from_numpy(P).to("cuda:0"), L.similarity(1.0, np.eye(3), [0, 0, 0]), err=err)
    assert abs(err[1].item() - float(th[1])) < 1e-6 * float(th[1]) and abs(float(th[1]) - 1e-9) < 1e-6 * 1e-9


def test_summary_sums_max_and_a_tie_across_workgroups(dev):
    """sums within the summation bound, max and argmax exact, and a tie for the maximum placed in two different workgroups returns the
    lower index -- with masks, and with the next set and its two counts"""
    D, L, ws, torch = dev["D"], dev["L"], dev["ws"], dev["torch"]
    n = 3 * 256 + 10
    x = noise_problem(0, n, seed=51)["pts"]
    y = A.move(x) + np.random.default_rng(3).normal(scale=1e-2, size=(n, 3))
    y[5] += [0.5, 0.0, 0.0]                                   # the largest error by far ...
    x[700], y[700] = x[5], y[5]                               # ... twice, in workgroups 0 and 2: the same inputs, the same bits
    sim = L.similarity(A.S0, A.R0, A.T0)
    base = np.ones(n, dtype=np.uint8)
    base[::7] = 0
    use = base.copy()
    use[1::5] = 0
    for b_, u_ in ((None, None), (base, use)):
        err = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        nxt = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
        tb, tu = (None if a is None else torch.from_numpy(a).to("cuda:0") for a in (b_, u_))
        out = D.align_errors_rows(ws, _rows4(dev, x), _rows4(dev, y), sim, base=tb, use=tu, max_dist=0.02, err=err, next_=nxt).cpu().numpy()
        e = err.cpu().numpy()
        ref = A.errors(x, y, A.S0, A.R0, A.T0)
        assert np.all(np.abs(e - ref) <= A.error_bound(x, y, A.S0, A.T0))
        assert e[5] == e[700] == e.max()
        on = np.ones(n, dtype=bool) if u_ is None else u_.astype(bool)
        S = A.summary(e, on)                                  # over the device's own errors: the sums' order is all that differs
        k = S["n"]
        assert out[0] == k and out[3] == e.max() and out[4] == 5
        assert abs(out[1] - S["sum_sq"]) <= (k + 8) * U * S["sum_sq"] and abs(out[2] - S["sum"]) <= (k + 8) * U * S["sum"]
        keep = (np.ones(n, dtype=bool) if b_ is None else b_.astype(bool)) & (e <= 0.02)
        assert np.array_equal(nxt.cpu().numpy(), keep.astype(np.uint8)) and out[5] == int((keep != on).sum()) and out[6] == int(keep.sum())
    off = np.zeros(n, dtype=np.uint8)
    out = D.align_errors_rows(ws, _rows4(dev, x), _rows4(dev, y), sim, use=torch.from_numpy(off).to("cuda:0")).cpu().numpy()
    assert list(out[:5]) == [0.0, 0.0, 0.0, -1.0, -1.0]         # nothing on


# ---- trimming -----------------------------------------------------------------------------------------------------------------------
def _centre_problem(c2b, c):
    """a problem whose camera centres are exactly c (identity rotations: c = -R^T t with R = I is exact), three points, no observation"""
    cams = np.zeros((len(c), 15))
    cams[:, [0, 4, 8]] = 1.0
    cams[:, 9:12] = -c
    cams[:, 12] = 1.0
    return _upload(c2b, cams, np.eye(3))


def test_trimming_follows_the_reference_round_by_round_and_equals_an_untrimmed_call_on_its_masks(c2b):
    x, y = A.dome_trim_case(5.0)
    est, ref = _centre_problem(c2b, x), _centre_problem(c2b, y)
    assert np.array_equal(est._camera_centers(), x) and np.array_equal(ref._camera_centers(), y)
    for rounds in (1, 2, 3):
        r = A.trim(x, y, 0.5, rounds)
        got = est.align(ref, max_dist=0.5, rounds=rounds, return_inliers=True, return_errors=True)
        assert got["status"] == "ok" and got["rounds"] == r["refits"]
        assert np.array_equal(got["camera_inliers"].astype(bool), r["final"]), rounds
        assert got["cameras"]["n"] == int(r["final"].sum())
        assert abs(got["scale"] - r["s"]) < 1e-12 and np.abs(got["rotation"] - r["R"]).max() < 1e-12
    assert sorted(np.flatnonzero(got["camera_inliers"] == 0)) == sorted(A.DOME_DISPLACED) and got["rounds"] == 2
    flat = est.align(ref, use_cameras=got["camera_inliers"], return_inliers=True, return_errors=True)       # one fit on the final masks
    assert flat["rounds"] == 0
    for k in ("scale", "rotation", "translation", "camera_errors", "camera_rotation_errors", "point_errors", "camera_inliers", "point_inliers"):
        assert np.array_equal(np.asarray(flat[k]), np.asarray(got[k])), k
    assert flat["cameras"] == got["cameras"] and flat["points"] == got["points"]
    # with a caller's mask: a correspondence that is off never comes back, whatever its distance
    mask = np.ones(len(x), dtype=np.uint8)
    mask[[0, 1, 2]] = 0
    r = A.trim(x, y, 0.5, 3, on=mask.astype(bool))
    got = est.align(ref, max_dist=0.5, rounds=3, use_cameras=mask, return_inliers=True)
    assert np.array_equal(got["camera_inliers"].astype(bool), r["final"]) and not got["camera_inliers"][:3].any() and got["rounds"] == r["refits"]


def test_trimming_reports_an_emptied_set(c2b):
    x, y = A.dome_trim_case(50.0)
    est, ref = _centre_problem(c2b, x), _centre_problem(c2b, y)
    first = est.align(ref)
    got = est.align(ref, max_dist=0.5, rounds=3, return_inliers=True)
    assert got["status"] == "too_few" and got["rounds"] == 0 and got["cameras"]["n"] == 0 and not got["camera_inliers"].any()
    for k in ("scale", "rotation", "translation"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(first[k])), k         # the first fit's transform, reported, not hidden
    few = est.align(ref, use_cameras=(np.arange(len(x)) < 2), return_inliers=True)
    assert few["status"] == "too_few" and few["scale"] == 1.0 and np.array_equal(few["rotation"], np.eye(3)) and not few["translation"].any()
    line = np.outer(np.arange(10.0), [1.0, 2.0, 3.0])
    deg = _centre_problem(c2b, line).align(_centre_problem(c2b, A.move(line)))
    assert deg["status"] == "degenerate" and deg["scale"] == 1.0 and np.array_equal(deg["rotation"], np.eye(3))
    flat = noise_problem(0, 40, seed=22, variant="planar")["pts"]
    pl = _centre_problem(c2b, flat).align(_centre_problem(c2b, A.move(flat)))        # rank 2 is not degenerate
    assert pl["status"] == "ok" and abs(pl["scale"] - A.S0) < 1e-12 and np.abs(pl["rotation"] - A.R0).max() < 1e-13


# ---- transform ------------------------------------------------------------------------------------------------------------------------
def _projection_bound(cams, pts, G, s, t):
    """|d uv| per observation of the moved problem against the original's.  The moved camera-frame point is s q + dq with |dq| <= 64u M,
    M = s max|x| + |t| the size of the moved coordinates: 8u M in X' and in c' (the transform's own bound), 4u per entry of R_c', the
    product t_c' = -R_c' c' and the projection's own R_c' X' + t_c' (each a three-term dot product of numbers up to M).  uv = -f r(p) p,
    p = q.xy / q.z: d uv <= f (1 + |p|) (1 + 3 |k1| |p|^2 + 5 |k2| |p|^4) |dq| / (s z) to first order, taken twice, + 16u |uv|."""
    rp = G["row_ptr"].astype(np.int64)
    ci = np.repeat(np.arange(len(cams)), np.diff(rp))
    Rm = cams[ci, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    q = np.einsum("nij,nj->ni", Rm, pts[G["pt_idx"].astype(np.int64)]) + cams[ci, 9:12]
    p = np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) / np.abs(q[:, 2])
    f, k1, k2 = cams[ci, 12], cams[ci, 13], cams[ci, 14]
    M = s * max(np.abs(pts).max(), np.abs(A.centers(cams).astype(np.float64)).max()) * np.sqrt(3.0) + np.linalg.norm(t)
    rad = 1 + np.abs(k1) * p ** 2 + np.abs(k2) * p ** 4
    return 2 * f * (1 + p) * (1 + 3 * np.abs(k1) * p ** 2 + 5 * np.abs(k2) * p ** 4) * 64 * U * M / (s * np.abs(q[:, 2])) + 16 * U * f * rad * p


def _transform_case(c2b, case):
    import oracle as O
    cams, pts, G = _truths()[case.split("-")[0]]
    if case == "dome-bal":
        return _upload(c2b, None, pts, G, bal9=G["true_bal9"]), O.camera_from_bal(G["true_bal9"]), pts, G
    return _upload(c2b, cams, pts, G), cams, pts, G


@pytest.mark.parametrize("case", ("dome-bal", "dome-state", "grid"))
def test_transform_against_the_reference(c2b, case):
    """points and centres within 8u (s |x| + |t|) of the reference, every camera orthonormal to 16u (largest entry of R^T R - I: a
    three-term dot product of entries <= 1, each 4u off), projections invariant within the bound above, the way back by align, the
    checkpoint, and the caches the table says are kept"""
    from city2ba_amd import _lib as L
    ba, cams, pts, G = _transform_case(c2b, case)
    orig = _upload(c2b, cams, pts, G)
    uv0 = ba.project()
    ba.covisibility(1)
    c_before, p_before = ba.cameras(), ba.points()
    ba.transform(A.S0, A.R0, A.T0)
    assert ba.covisibility_heavy_cameras() is not None        # the graph's handle survived (the list did not change)
    rc, rp_ = A.apply(c_before, p_before, A.S0, A.R0, A.T0)
    gc, gp = ba.cameras(), ba.points()
    bp = 8 * U * (A.S0 * np.linalg.norm(p_before, axis=1) + np.linalg.norm(A.T0))
    assert np.all(np.linalg.norm(gp - rp_, axis=1) <= bp)
    x = A.centers(c_before).astype(np.float64)
    bc = 8 * U * (A.S0 * np.linalg.norm(x, axis=1) + np.linalg.norm(A.T0))
    assert np.all(np.linalg.norm(A.centers(gc).astype(np.float64) - A.centers(rc).astype(np.float64), axis=1) <= bc + 8 * U * np.linalg.norm(A.centers(rc).astype(np.float64), axis=1))
    assert np.all(np.linalg.norm(ba._camera_centers() - A.centers(rc).astype(np.float64), axis=1) <= bc + 8 * U * np.linalg.norm(A.centers(rc).astype(np.float64), axis=1))
    Rm = gc[:, :9].reshape(-1, 3, 3).astype(A.LD)
    assert float(np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max()) < 16 * U
    assert np.array_equal(gc[:, 12:], c_before[:, 12:])      # f, k1, k2 untouched
    uv1 = ba.project()                                        # (the camera table was rebuilt: a stale one would project the old frame)
    assert np.all(np.linalg.norm(uv1 - uv0, axis=1) <= _projection_bound(c_before, p_before, G, A.S0, A.T0))
    back = ba.align(orig, on="both")
    sel = (np.concatenate([ba._camera_centers(), gp]), np.concatenate([orig._camera_centers(), pts]))
    st, s, R, t, sig, eps = A.fit(*sel)
    m = A.moments(*sel)
    dR, ds, dt = A.fit_bounds(m, sig, eps, s, _d_sigma(m), (m["n"] + 8) * U)
    assert np.sqrt(((back["rotation"] - R) ** 2).sum()) <= dR and abs(back["scale"] - s) <= ds and np.linalg.norm(back["translation"] - t) <= dt
    # the composition is the identity up to what the moved data's rounding (eps per entity) allows the fit: eps / spread, first order
    eps_d, spread = max(bp.max(), bc.max()), float(np.sqrt(sig[1] / s))
    assert abs(back["scale"] * A.S0 - 1) <= 4 * eps_d / spread + ds * A.S0
    assert np.sqrt(((back["rotation"] @ A.R0 - np.eye(3)) ** 2).sum()) <= 4 * eps_d / spread + dR
    assert np.linalg.norm(back["scale"] * back["rotation"] @ A.T0 + back["translation"]) <= 4 * eps_d * (1 + np.linalg.norm(m["mean_x"].astype(np.float64)) / spread) + dt
    assert back["cameras"]["max"] <= 2 * bc.max() + dt + 1e-13 and back["points"]["max"] <= 2 * bp.max() + dt + 1e-13
    # a checkpoint around a transform restores the bits (the checkpoint itself takes a state-mode problem to bal mode first)
    ba.checkpoint()
    c_ck, p_ck, uv_ck = ba.cameras(), ba.points(), ba.project()
    ba.transform(0.5, A.R0.T, -A.T0)
    assert not np.array_equal(ba.points(), p_ck)
    ba.rollback()
    assert np.array_equal(ba.cameras(), c_ck) and np.array_equal(ba.points(), p_ck) and np.array_equal(ba.project(), uv_ck)


def test_refusals_write_nothing_and_align_leaves_both_problems_untouched(c2b):
    from city2ba_amd import _lib as L
    cams, pts, G = _truths()["dome"]
    ba, ref = _upload(c2b, cams, pts, G), _upload(c2b, cams, pts, G)
    small = _upload(c2b, cams[:-1], pts)
    before = (ba.cameras(), ba.points(), ba.cameras_bal(), ref.cameras(), ref.points())
    with pytest.raises(c2b.City2baError) as ei:
        ba.align(small)
    assert ei.value.status == L.ERR_INVALID_ARGUMENT and "sizes differ" in str(ei.value)
    L.check(L.lib().c2b_problem_set_shard(ref._h, 0, len(cams) + 5, 0))
    for call in (lambda: ba.align(ref), lambda: ref.align(ba), lambda: ref.transform(1.0, np.eye(3), np.zeros(3))):
        with pytest.raises(c2b.City2baError) as ei:
            call()
        assert ei.value.status == L.ERR_INVALID_ARGUMENT and "shard" in str(ei.value)
    for s, R in ((0.0, np.eye(3)), (float("nan"), np.eye(3)), (1.0, np.diag([1.0, 1.0, -1.0])), (1.0, np.eye(3) + 1e-8), (1.0, 2 * np.eye(3))):
        with pytest.raises(c2b.City2baError) as ei:
            ba.transform(s, R, np.zeros(3))
        assert ei.value.status == L.ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        ba.align(ref, on="everything")
    ref2 = _upload(c2b, cams, pts, G)
    ba.align(ref2, on="both", max_dist=0.5, rounds=2, return_errors=True, return_inliers=True)
    after = (ba.cameras(), ba.points(), ba.cameras_bal(), ref.cameras(), ref.points())
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(ref2.cameras(), cams) and np.array_equal(ref2.points(), pts)


def test_fifty_align_and_transform_pairs_leave_the_free_memory_where_it_was(c2b):
    import torch
    cams, pts, G = _truths()["grid"]
    ba, ref = _upload(c2b, cams, pts, G), _upload(c2b, cams, pts, G)
    Rb = A.rotation([1.0, 2.0, 3.0], 0.01)

    def pair():
        ba.align(ref, on="both", max_dist=1.0, rounds=2, return_errors=True, return_inliers=True)
        ba.transform(1.001, Rb, [0.1, 0.2, 0.3])
    pair()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(50):
        pair()
    torch.cuda.synchronize()
    drop = free0 - torch.cuda.mem_get_info(0)[0]
    print("free device memory dropped by %d bytes over 50 align + transform pairs" % drop)
    assert drop <= 0


def test_a_free_gauge_solve_comes_closer_to_the_truth(c2b):
    """dome_problem(obs_noise=0) solved by the device LM loop with nothing held constant and no priors -- the gauge is free -- and compared
    against the true problem: the camera RMSE after alignment must fall strictly below the start's"""
    import oracle as O
    from city2ba_amd import solve
    d = dome_problem(seed=0, obs_noise=0.0)
    ba = c2b.BAProblem.from_bal(d["bal9"], d["pts"], d["row_ptr"], d["pt_idx"], d["uv"])
    truth = c2b.BAProblem.from_bal(d["true_bal9"], d["true_pts"], d["row_ptr"], d["pt_idx"], d["uv"])
    start = solve.compare(ba, truth, on="cameras")
    history, summary = solve.levenberg_marquardt_device(ba, iterations=20)
    end = solve.compare(ba, truth, on="cameras")
    print("camera RMSE after alignment: start %.6g, after %d LM iterations %.6g (cost %.6g -> %.6g); points %.6g -> %.6g"
          % (start["cameras"]["rmse"], len(history), end["cameras"]["rmse"], summary["initial_cost"], summary["final_cost"],
             start["points"]["rmse"], end["points"]["rmse"]))
    assert start["status"] == end["status"] == "ok"
    assert end["cameras"]["rmse"] < start["cameras"]["rmse"]
