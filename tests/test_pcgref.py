"""The reference PCG of tests/_schurref.py (pcg) checked on the CPU: it reaches the dense Schur solve, with M = I it is
textbook CG, an f64 restatement of c2b_problem_solve_step's loop in the device's order (its factorisation, its triangular
solves, its reduction trees) stays inside the per-iterate bounds, and restated mutations of that loop land far outside."""
import numpy as np
import pytest

import _schurref as R

LD = R.LD


def _random(seed, n_cam=12, n_pts=40, n_obs=160, dtype=np.float64):
    """random r / Jc / Jp on a random list (uneven columns like f, k1, k2); camera 0 and point 3 never observed"""
    rng = np.random.default_rng(seed)
    cam_of = np.sort(rng.choice(np.arange(1, n_cam), n_obs))
    pt_idx = rng.choice(np.setdiff1d(np.arange(n_pts), [3]), n_obs)
    scale = np.array([1.0, 1.0, 1.0, 0.1, 0.1, 0.1, 1e-3, 10.0, 100.0])
    Jc = rng.normal(size=(n_obs, 2, 9)) * scale
    Jp = rng.normal(size=(n_obs, 2, 3))
    r = rng.normal(size=(n_obs, 2))
    return R.Problem(r, Jc, Jp, cam_of, pt_idx, n_cam, n_pts, dtype=dtype)


def _ld(P):
    return R.Problem(P.r, P.Jc, P.Jp, P.cam, P.pt, P.n_cam, P.n_pts, dtype=LD)


# ---- the device's loop in f64, in the device's order -----------------------------------------------------------------
def _wave_sum(v):
    """wave_sum: lane 0 of the shfl_down tree over the last axis (64 lanes)"""
    off = 32
    while off:
        v = v[..., :off] + v[..., off:2 * off]
        off >>= 1
    return v[..., 0]


def _block_sum(v):
    """block_sum_to over 256 threads: four wave trees, then ((w0 + w1) + w2) + w3"""
    w = _wave_sum(v.reshape(v.shape[:-1] + (4, 64)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _normal_sum(parts):
    """k_normal_sum: thread t adds partials t, t + 256, ... in turn, then the workgroup's tree"""
    n = len(parts)
    m = -(-n // 256)
    a = np.zeros(256)
    pad = np.zeros(m * 256)
    pad[:n] = parts
    for row in pad.reshape(m, 256):
        a = a + row
    return _block_sum(a)


class DeviceF64:
    """c2b_problem_solve_step's arithmetic in f64: the operator of an f64 Problem, k_schur_factor / chol9_solve in their
    order with reciprocal pivots, k_schur_cameras<kSchurDot>'s wave partials of p.q, k_pcg_update's per-thread and
    per-workgroup r.r / r.z, k_normal_sum, x + alpha p without contraction.  `mut` restates one mutation:
    M1 the factor damps with lam / 2, M2 z = r, M3 the loop's r.r sums one workgroup's partial, M4 (pcg_loop's
    beta_scale), M5 the p.q partial drops each wave's fourth camera."""

    def __init__(self, P, lam, mut=None):
        self.P, self.lam, self.mut = P, lam, mut
        nc = P.n_cam
        U = P.U.astype(np.float64)
        flam = lam / 2 if mut == "M1" else lam
        a = {}
        for i in range(9):
            for j in range(i + 1):
                a[i, j] = R.damp_diag(U[:, i, j], flam) if i == j else U[:, i, j].copy()
        for j in range(9):
            d = a[j, j]
            for k in range(j):
                d = d - a[j, k] * a[j, k]
            inv = 1.0 / np.sqrt(d)
            a[j, j] = inv
            for i in range(j + 1, 9):
                v = a[i, j]
                for k in range(j):
                    v = v - a[i, k] * a[j, k]
                a[i, j] = v * inv
        self.l = a
        self.nbc = -(-nc // 256)
        quads = -(-nc // 4)
        self.n_waves = -(-quads // 4) * 4

    def zeros_like(self, v):
        return np.zeros_like(v)

    def sqrt(self, v):
        return np.sqrt(v)

    def div(self, a, b):
        return np.float64(a) / np.float64(b)

    def rhs(self):
        return np.asarray(self.P.rhs(self.lam)[0], dtype=np.float64)

    def S(self, p):
        return np.asarray(self.P.S_times(self.lam, p)[0], dtype=np.float64)

    def precond(self, r):
        if self.mut == "M2":
            return r.copy()
        l, z = self.l, np.zeros_like(r)
        for i in range(9):
            v = r[:, i]
            for k in range(i):
                v = v - l[i, k] * z[:, k]
            z[:, i] = v * l[i, i]
        for i in range(8, -1, -1):
            v = z[:, i]
            for k in range(i + 1, 9):
                v = v - l[k, i] * z[:, k]
            z[:, i] = v * l[i, i]
        return z

    def dot_pq(self, p, q):
        lanes = np.zeros((self.n_waves * 4, 16))
        lanes[:len(p), :9] = p * q
        if self.mut == "M5":
            lanes[3::4] = 0.0
        return _normal_sum(_wave_sum(lanes.reshape(self.n_waves, 64)))

    def dot_rr(self, a, b, loop=False):
        t = np.zeros(self.nbc * 256)
        s = np.zeros(len(a))
        for k in range(9):
            s = s + a[:, k] * b[:, k]
        t[:len(a)] = s
        parts = _block_sum(t.reshape(self.nbc, 256))
        if loop and self.mut == "M3":
            parts = parts[:1]
        return _normal_sum(parts)

    def axpy(self, y, a, x):
        return y + a * x


def device_f64(P64, lam, max_iters, rel_tol, mut=None):
    return R.pcg_loop(DeviceF64(P64, lam, mut), max_iters, rel_tol, beta_scale=0.9 if mut == "M4" else 1.0)


def _over(err, bound):
    return err / bound if bound > 0 else (0.0 if err == 0 else np.inf)


def _ratios(ref, got, P, lam):
    """per iterate |err| / bound of x, dp, the recurrence's |r_k| / |b| and the energy"""
    out = dict(x=[], dp=[], rel=[], energy=[])
    P64 = R.Problem(P.r, P.Jc, P.Jp, P.cam, P.pt, P.n_cam, P.n_pts)
    for k in range(min(len(ref["x"]), len(got["xs"]))):
        x = got["xs"][k]
        dp = np.asarray(P64.back_substitute(lam, x)[0], dtype=np.float64)
        b = ref["bound"]
        out["x"].append(_over(np.linalg.norm(x - ref["x"][k].astype(np.float64)), b["x"][k]))
        out["dp"].append(_over(np.linalg.norm(dp - ref["dp"][k].astype(np.float64)), b["dp"][k]))
        out["rel"].append(_over(abs(float(got["rel"][k]) - float(ref["rel"][k])), b["rel"][k]))
        out["energy"].append(_over(abs(float(R.energy(P, lam, x) - ref["energy"][k])), b["energy"][k]))
    return {k: np.array(v) for k, v in out.items()}


# ---- 1. the reference reaches the dense Schur solve -------------------------------------------------------------------
@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_reference_pcg_reaches_the_dense_schur_solve(lam):
    P64 = _random(1)
    P = _ld(P64)
    ref = R.pcg(P, lam, 400, 1e-15, runs=0)
    assert ref["status"] == 0 and ref["rel_residual"] <= 1e-15, (ref["status"], ref["iterations"])
    dc, dp = P64.schur_direct(lam)
    x = ref["x"][-1].astype(np.float64)
    assert np.linalg.norm(x - dc) <= 1e-9 * np.linalg.norm(dc)
    assert np.linalg.norm(ref["dp"][-1].astype(np.float64) - dp) <= 1e-9 * np.linalg.norm(dp)
    # the energy never rises, falls strictly while the residual is above 1e-6, and ends at -1/2 b^T S^-1 b
    en = np.array([float(e) for e in ref["energy"]])
    rel = np.array([float(v) for v in ref["rel"]])
    assert (np.diff(en) <= 1e-15 * abs(en[-1])).all() and (np.diff(en)[rel[:-1] > 1e-6] < 0).all()
    b, _ = P.rhs(lam)
    assert abs(en[-1] + 0.5 * float(np.sum(b.astype(np.float64) * dc))) <= 1e-9 * abs(en[-1])


def test_identity_preconditioner_is_textbook_cg():
    P = _ld(_random(2))
    lam = 1e-2
    ops = R._pcg_ops(P, lam)
    ops.Minv = np.broadcast_to(np.eye(9, dtype=LD), ops.Minv.shape)
    got = R.pcg_loop(ops, 12, 0.0)
    # Hestenes-Stiefel, written out
    b, _ = P.rhs(lam)
    x, r = np.zeros_like(b), b.copy()
    p, rr = r.copy(), np.sum(r * r)
    for k in range(1, 13):
        q, _ = P.S_times(lam, p)
        alpha = rr / np.sum(p * q)
        x, r = x + alpha * p, r - alpha * q
        rr_new = np.sum(r * r)
        p, rr = r + (rr_new / rr) * p, rr_new
        assert np.linalg.norm((got["xs"][k] - x).astype(np.float64)) <= 1e-15 * np.linalg.norm(x.astype(np.float64)), k
        assert abs(float(got["rel"][k] - np.sqrt(rr) / np.sqrt(np.sum(b * b)))) <= 1e-15


# ---- 2. the device's order inside the bound; mutations far outside ----------------------------------------------------
CASES = [(3, 12, 40, 160, 1e-4), (4, 12, 40, 160, 1.0), (5, 30, 200, 700, 1e-3), (6, 520, 900, 3000, 1e-2)]


@pytest.fixture(scope="module")
def cases():
    out = []
    for seed, nc, npt, no, lam in CASES:
        P64 = _random(seed, nc, npt, no)
        P = _ld(P64)
        out.append((P64, P, lam, R.pcg(P, lam, 13, 0.0, seed=seed)))
    return out


def test_device_order_f64_stays_inside_the_bound(cases):
    worst = {}
    for P64, P, lam, ref in cases:
        got = device_f64(P64, lam, 13, 0.0)
        assert got["status"] == 1 and got["iterations"] == 13
        rat = _ratios(ref, got, P, lam)
        for k, v in rat.items():
            worst[k] = max(worst.get(k, 0.0), float(v.max()))
            assert (v <= 1.0).all(), (P.n_cam, lam, k, v)
    print("worst |err| / bound of the f64 restatement:", worst)


@pytest.mark.parametrize("mut", ["M1", "M2", "M3", "M4", "M5"])
def test_mutations_land_far_outside_the_bound(cases, mut):
    worst = 0.0
    for P64, P, lam, ref in cases:
        rat = _ratios(ref, device_f64(P64, lam, 13, 0.0, mut), P, lam)
        worst = max(worst, max(float(v.max()) for v in rat.values()))
    print(mut, "worst |err| / bound:", worst)
    assert worst >= 100.0, (mut, worst)
