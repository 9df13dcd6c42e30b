"""Host reference of the direct solve of the reduced camera system: the dense image, a blocked Cholesky, the two
substitutions and the bounds a device factor and solution are held to.  numpy only, longdouble where it says so.

The semantics, restated from include/city2ba_hip_experimental.h:
  * c2b_problem_set_linear_solver chooses pcg (0, the default) or cholesky (1) per handle; it is not a value of set_schur.  Under
    cholesky solve_step forms S as the explicit path does whatever `schur` says (the pattern, then S_diag / S_off without the
    preconditioner's factors, b by the implicit pass), ignores the preconditioner, and reports 0 fallbacks.
  * The dense image: N = 9 n_cam, Np = 64 ceil(N / 64), A row-major with leading dimension Np; only the lower triangle, diagonal
    included, is meaningful -- the upper triangle is never read and unspecified afterwards; the padding rows i >= N hold 1 on
    the diagonal and 0 elsewhere.  linear_solver_bytes = 8 (schur_explicit_doubles + Np^2 + 2 Np); more than 4096 cameras are
    refused.
  * A constant entry's row and column of S are exactly 0 with lambda 1e-6 on the diagonal, an empty camera's block is lambda 1e-6 I,
    b is exactly 0 there and the substitutions return exactly +0.0 there.
  * The result: 0 iterations; status 0 when every pivot was finite and > 0, else 2 with dc = dp = 0, rel_residual 1 and
    model_decrease 0; rel_residual is the true |b - S dc| / |b| (0 when b = 0); the same problem and arguments give the same bits.
  * A pivot that is not finite or not > 0 leaves its 1-based index in info (the first one only) and is replaced by 1.

The bounds (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorems 10.3 and 10.4; they hold for any order of
summation and with fused multiply-adds), u = 2^-53, gamma_k = k u / (1 - k u), L the COMPUTED factor, entry by entry:
  |A - L L^T| <= gamma_{n+1} |L| |L^T|                 (factor_excess)
  |b - A x|   <= gamma_{3n+1} |L| |L^T| |x|            (solve_excess)
Both sides are evaluated in longdouble, whose own rounding (2^-64 per operation) is 2^-11 of u."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TILE = 64


def padded(n):
    return (n + TILE - 1) // TILE * TILE


def gamma(k):
    return LD(k) * LD(U) / (1 - LD(k) * LD(U))


def lower_image(S, dtype=np.float64):
    """the dense image of a symmetric S [N, N]: its lower triangle in [Np, Np], zeros above it, identity padding rows"""
    n = len(S)
    A = np.zeros((padded(n), padded(n)), dtype=dtype)
    A[:n, :n] = np.tril(np.asarray(S, dtype=dtype))
    i = np.arange(n, padded(n))
    A[i, i] = 1
    return A


def assemble(nbr_ptr, nbr, D, E, dtype=np.float64):
    """the blocks (D [n_cam, 9, 9] on the diagonal, E [n_edges, 9, 9] at block column nbr[e] of the row that holds e) as S [9 n_cam,
    9 n_cam] in `dtype`: _explicitref.dense without its cast"""
    n_cam = len(D)
    S = np.zeros((9 * n_cam, 9 * n_cam), dtype=dtype)
    row = np.repeat(np.arange(n_cam), np.diff(np.asarray(nbr_ptr).astype(np.int64)))
    for c in range(n_cam):
        S[9 * c:9 * c + 9, 9 * c:9 * c + 9] = D[c]
    for e, (c, q) in enumerate(zip(row, np.asarray(nbr).astype(np.int64))):
        S[9 * c:9 * c + 9, 9 * q:9 * q + 9] = E[e]
    return S


def image_of_blocks(nbr_ptr, nbr, D, E):
    """what c2b_dense_scatter_rows leaves in the lower triangle, padding included (float64; copies, no arithmetic)"""
    return lower_image(assemble(nbr_ptr, nbr, np.asarray(D, dtype=np.float64), np.asarray(E, dtype=np.float64)))


def cholesky(A, n=None):
    """(L, info): the right-looking blocked Cholesky of the lower triangle of A [Np, Np] on 64 x 64 tiles, in A's dtype -- the
    diagonal tile column by column, the tiles below it by substitution (X L11^T = A21, no inverse), the trailing lower tiles
    minus the panel's product.  info = the 1-based index of the first pivot that is not finite or not > 0 (0: none); such a pivot
    is replaced by 1.  The upper triangle of L is 0.  n is not needed: padding rows are rows like any other."""
    L = np.tril(np.array(A, copy=True))
    Np = len(L)
    assert Np % TILE == 0 and L.shape == (Np, Np)
    info = 0
    one = L.dtype.type(1)
    for k0 in range(0, Np, TILE):
        k1 = k0 + TILE
        for j in range(k0, k1):                                  # the panel, column by column
            d = L[j, j]
            ok = bool(np.isfinite(d)) and d > 0
            if not ok and not info:
                info = j + 1
            piv = np.sqrt(d) if ok else one
            L[j, j] = piv
            L[j + 1:k1, j] = L[j + 1:k1, j] / piv
            col = L[j + 1:k1, j]
            L[j + 1:k1, j + 1:k1] -= np.tril(np.outer(col, col))
        if k1 == Np:
            break
        for j in range(k0, k1):                                  # X L11^T = A21, column j of X after its predecessors
            L[k1:, j] = (L[k1:, j] - L[k1:, k0:j] @ L[j, k0:j]) / L[j, j]
        P = L[k1:, k0:k1]
        L[k1:, k1:] -= np.tril(P @ P.T)
    return L, info


def solve(L, b):
    """x = L^-T L^-1 b by forward and backward substitution in L's dtype"""
    n = len(L)
    y = np.array(b, dtype=L.dtype, copy=True).reshape(n)
    for i in range(n):
        y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - L[i + 1:, i] @ y[i + 1:]) / L[i, i]
    return y


def _ld(M):
    return np.asarray(M, dtype=np.float64).astype(LD)


def factor_excess(A, L, n):
    """max over the lower triangle of |A - L L^T| / (gamma_{n+1} |L| |L^T|), entry by entry in longdouble; an entry whose bound is 0
    must be met exactly (inf otherwise).  A and L are the image [Np, Np] before and after; n the matrix's order."""
    A, L = np.tril(_ld(A)), np.tril(_ld(L))
    err = np.abs(A - np.tril(L @ L.T))
    bound = gamma(n + 1) * np.tril(np.abs(L) @ np.abs(L).T)
    return _worst(err, bound, np.tril(np.ones(A.shape, dtype=bool)))


def solve_excess(A, L, x, b, n):
    """max over the entries of |b - A x| / (gamma_{3n+1} |L| |L^T| |x|) in longdouble; A the symmetric matrix its lower image
    stands for"""
    A, L, x, b = np.tril(_ld(A)), np.tril(_ld(L)), _ld(x).reshape(-1), _ld(b).reshape(-1)
    full = A + np.tril(A, -1).T
    err = np.abs(b - full @ x)
    bound = gamma(3 * n + 1) * (np.abs(L) @ (np.abs(L).T @ np.abs(x)))
    return _worst(err, bound, np.ones(len(x), dtype=bool))


def _worst(err, bound, where):
    err, bound = err[where], bound[where]
    if np.any((bound == 0) & (err != 0)) or not np.all(np.isfinite(err)):
        return np.inf
    pos = bound > 0
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


def spd(n, seed, scaled=False):
    """G G^T + n I with seeded uniform G in [-1, 1) (float64, rounded once); scaled: D (.) D with D = diag(10^u), u uniform in
    [-3, 3] -- symmetric in float64 by construction"""
    rng = np.random.default_rng(seed)
    G = rng.uniform(-1.0, 1.0, size=(n, n))
    A = G @ G.T + n * np.eye(n)
    A = (A + A.T) / 2
    if scaled:
        d = 10.0 ** rng.uniform(-3.0, 3.0, size=n)
        A = A * d[:, None] * d[None, :]
        A = np.tril(A) + np.tril(A, -1).T
    return A


# ---- the step ---------------------------------------------------------------------------------------------------------------
LD_DIRECT_MAX = 320         # up to this order solve_ld factors in longdouble; above it, it refines an f64 solve (numpy's longdouble
                            # matrix product runs at ~0.2 GFLOP/s: the dome's 720 take seconds per factorisation, and a bound takes nine);
                            # tests/test_denseref.py holds the one to the other on the dome


def solve_refined(S, b):
    """x with S x = b to longdouble accuracy for a symmetric positive definite S in longdouble: an f64 inverse as the approximate
    solver, residuals b - S x in longdouble.  The correction contracts by ~cond(S) 2^-53 per round until it reaches the level of
    the longdouble residual's own rounding, ~cond(S) 2^-64 of x, which is also what a longdouble factorisation leaves: it stops
    below 2^-60 of x, or when the correction stops shrinking below 2^-45 of x"""
    S, b = np.asarray(S, dtype=LD), np.asarray(b, dtype=LD).reshape(-1)
    Si = np.linalg.inv(S.astype(np.float64))
    x = np.zeros(len(b), dtype=LD)
    prev = np.inf
    for _ in range(40):
        dx = (Si @ (b - S @ x).astype(np.float64)).astype(LD)
        x = x + dx
        step, size = np.linalg.norm(dx.astype(np.float64)), np.linalg.norm(x.astype(np.float64))
        if step <= 2.0 ** -60 * size or (step > 0.25 * prev and step <= 2.0 ** -45 * size):
            return x
        prev = step
    raise AssertionError("solve_refined: no convergence (the system is too ill-conditioned for an f64 inverse)")


def solve_ld(S, b, how=None):
    """the longdouble solution of S x = b: how = "cholesky" (the blocked factorisation above, in longdouble), "refined"
    (solve_refined), None = by the order"""
    n = len(S)
    if how == "refined" or (how is None and n > LD_DIRECT_MAX):
        return solve_refined(S, b)
    L, info = cholesky(lower_image(np.asarray(S, dtype=LD), dtype=LD))
    assert info == 0
    return solve(L, np.concatenate([np.asarray(b, dtype=LD).reshape(-1), np.zeros(len(L) - n, dtype=LD)]))[:n]


def direct_step(P, lam, rng=None, how=None):
    """(dc [n_cam, 9], dp [n_pts, 3]) of the _schurref.Problem P (longdouble) by the direct solve of its reduced system: S from
    _explicitref.blocks (under rng one perturbed f64-like evaluation of them), b = P.rhs (under rng moved by its scale),
    solve_ld, the back-substitution"""
    import _explicitref as X
    B = X.blocks(P, lam, rng)
    S = assemble(B["nbr_ptr"], B["nbr"], B["D"], B["E"], dtype=LD)
    b, bscale = P.rhs(lam)
    b = X._jig(b, bscale, rng)
    dc = solve_ld(S, b, how).reshape(P.n_cam, 9)
    dp, dscale = P.back_substitute(lam, dc)
    return dc, X._jig(dp, dscale, rng)


def direct_step_bound(P, lam, runs=8, seed=0, mult=16.0, floor=1e-13, how=None):
    """dict(x, dp, bound_x, bound_dp): the longdouble direct step and what an f64 evaluation is held to in the 2-norm, by the
    project's rule (_explicitref.pcg's): `mult` x the largest deviation over `runs` seeded perturbed reruns, which perturb S and b
    by _explicitref.blocks' model and then solve them directly, floored at `floor` x the norm"""
    assert P.dtype == LD
    x, dp = direct_step(P, lam, how=how)
    rng = np.random.default_rng(seed)
    dev_x = dev_dp = 0.0
    norm = lambda v: float(np.linalg.norm(np.asarray(v).astype(np.float64)))
    for _ in range(runs):
        px, pdp = direct_step(P, lam, rng, how=how)
        dev_x, dev_dp = max(dev_x, norm(px - x)), max(dev_dp, norm(pdp - dp))
    return dict(x=x, dp=dp, bound_x=max(mult * dev_x, floor * norm(x)), bound_dp=max(mult * dev_dp, floor * norm(dp)),
                deviation=(dev_x, dev_dp))
