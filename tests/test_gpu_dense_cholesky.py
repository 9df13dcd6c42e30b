"""Level 0 of the direct solver on the device: c2b_dense_cholesky and c2b_dense_cholesky_solve at the tile edges of the
four factor kernels and at the dome's size, held entry by entry to the backward-error bounds of a Cholesky factorisation and of the
two substitutions (tests/_denseref.py: Higham, Thms 10.3 and 10.4 -- derived, not measured, and valid for any summation order and
for fused multiply-adds, so for the MFMA's k-chain too); the padding rows, the reported pivot, two runs the same bits; and
c2b_dense_scatter_rows against _explicitref.dense bit for bit.  A failed pivot is a numerical status: nothing here provokes a fault."""
import numpy as np
import pytest

import _covisref as CR
import _denseref as DR
import _explicitref as X
from test_gpu_coupled import _dome, _load
from test_gpu_schur_explicit import _list_problem
from test_gpu_schur_step import _bits, _np, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
SIZES = [1, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193, 729]


def _poisoned(img):
    """the image with NaN above the diagonal: the upper triangle is never read"""
    A = img.copy()
    A[np.triu_indices(len(A), 1)] = np.nan
    return A


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_factor_and_solution_meet_the_backward_error_bounds(env, n, scaled):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    A = DR.spd(n, seed=n, scaled=scaled)
    img = DR.lower_image(A)
    Np = DR.padded(n)
    b = np.zeros(Np)
    b[:n] = np.random.default_rng(1000 + n).normal(size=n)
    runs = []
    for _ in range(2):
        d_A = torch.from_numpy(_poisoned(img)).to(dev)
        d_x = torch.from_numpy(b.copy()).to(dev)
        info = torch.full((1,), -5, dtype=torch.int32, device=dev)
        D.dense_cholesky(d_A, n, info)
        D.dense_cholesky_solve(d_A, n, d_x)
        torch.cuda.synchronize()
        runs.append((_np(d_A).copy(), _np(d_x).copy(), int(_np(info)[0])))
    got, x, status = runs[0]
    assert status == 0
    L = np.tril(got)
    assert np.isfinite(L).all() and np.isnan(got[np.triu_indices(Np, 1)]).all()      # the upper triangle was not written either
    assert _bits(L[n:], np.eye(Np)[n:])                                              # padding rows are left as identity rows
    assert _bits(np.tril(runs[1][0]), L) and _bits(runs[1][1], x) and runs[1][2] == 0        # two runs: the same bits
    fe = DR.factor_excess(img[:n, :n], L[:n, :n], n)
    se = DR.solve_excess(img[:n, :n], L[:n, :n], x[:n], b[:n], n)
    print("DENSE cholesky n=%d scaled=%d: |A - L L^T| / (gamma_%d |L||L^T|) %.3g, |b - A x| / (gamma_%d |L||L^T||x|) %.3g"
          % (n, scaled, n + 1, fe, 3 * n + 1, se))
    assert fe <= 1.0, (n, scaled, fe)
    assert se <= 1.0, (n, scaled, se)
    assert not x[n:].any()


def test_leading_dimension_beyond_the_padded_order(env):
    """ld = Np + 64: the same factor and solution, bit for bit, and nothing written past column Np"""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    n = 129
    img = DR.lower_image(DR.spd(n, seed=n))
    Np = DR.padded(n)
    b = np.zeros(Np)
    b[:n] = np.random.default_rng(1000 + n).normal(size=n)
    out = []
    for ld in (Np, Np + 64):
        wide = np.full((Np, ld), np.nan)
        wide[:, :Np] = _poisoned(img)
        d_A, d_x = torch.from_numpy(wide).to(dev), torch.from_numpy(b.copy()).to(dev)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        D.dense_cholesky(d_A, n, info)
        D.dense_cholesky_solve(d_A, n, d_x)
        torch.cuda.synchronize()
        got = _np(d_A)
        assert np.isnan(got[:, Np:]).all() and int(_np(info)[0]) == 0
        out.append((np.tril(got[:, :Np]).copy(), _np(d_x).copy()))
    assert _bits(out[0][0], out[1][0]) and _bits(out[0][1], out[1][1])


@pytest.mark.parametrize("bad", [-1.0, float("nan")])
@pytest.mark.parametrize("k", [0, 63, 64, 100])
def test_first_failing_pivot_is_reported_and_the_factorisation_runs_to_its_end(env, k, bad):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    n = 193
    A = np.eye(n)
    A[k, k] = bad
    A[150, 150] = -2.0                                                               # a later failure: only the first is kept
    img = DR.lower_image(A)
    want, winfo = DR.cholesky(img)
    assert winfo == k + 1
    d_A = torch.from_numpy(_poisoned(img)).to(dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    D.dense_cholesky(d_A, n, info)
    torch.cuda.synchronize()
    assert int(_np(info)[0]) == k + 1
    assert _bits(np.tril(_np(d_A)), want)                                            # it went on with a pivot of 1: the identity
    info.fill_(9)                                                                    # a good matrix afterwards: info is set to 0 first
    d_A = torch.from_numpy(_poisoned(DR.lower_image(np.eye(n)))).to(dev)
    D.dense_cholesky(d_A, n, info)
    torch.cuda.synchronize()
    assert int(_np(info)[0]) == 0


def _scatter_case(which):
    if which == "dome":
        return _load(_dome("bal"))
    if which == "empty list":
        row_ptr, pt_idx = CR._lists([[], [], []])
        return _list_problem(row_ptr, pt_idx, 7, seed=3)
    degree = int(which.split()[1])
    row_ptr, pt_idx, n_pts = CR.hub_list(degree, False)
    return _list_problem(row_ptr, pt_idx, n_pts, seed=degree)


@pytest.mark.parametrize("which", ["dome", "hub 1", "hub 63", "hub 64", "hub 65", "empty list"])
def test_scatter_is_the_assembled_lower_triangle_bit_for_bit(env, which):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    ba = _scatter_case(which)
    lam = 1e-2
    nbr_ptr, nbr, Sd, So, _ = ba.schur_complement(lam)
    nc = len(Sd)
    n, Np = 9 * nc, DR.padded(9 * nc)
    if which.startswith("hub"):
        assert np.diff(nbr_ptr.astype(np.int64)).max() == int(which.split()[1])
    if which == "empty list":
        assert len(nbr) == 0 and ba.num_observations() == 0
    want = np.zeros((Np, Np))
    want[:n, :n] = np.tril(X.dense(dict(nbr_ptr=nbr_ptr, nbr=nbr, D=Sd, E=So), nc))
    want[np.arange(n, Np), np.arange(n, Np)] = 1.0
    assert _bits(want, DR.image_of_blocks(nbr_ptr, nbr, Sd, So))
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else a.view(dt))).to(dev)
    d_ptr, d_nbr = t(nbr_ptr, np.int64), t(nbr if len(nbr) else np.zeros(1, dtype=np.uint32), np.int32)
    d_Sd, d_So = t(Sd), t(So if len(So) else np.zeros((1, 9, 9)))
    for ld in (Np, Np + 64):
        A = torch.full((Np, ld), float("nan"), dtype=torch.float64, device=dev)
        D.dense_scatter_rows(d_ptr, d_nbr, d_Sd, d_So, A)
        torch.cuda.synchronize()
        got = _np(A)
        assert _bits(np.tril(got[:, :Np]), want), (which, ld)
        assert np.isnan(got[:, Np:]).all()
        above = got[:, :Np][np.triu_indices(Np, 9)]                                  # beyond a diagonal block nothing is written
        assert np.isnan(above).all()
    ba.close()
