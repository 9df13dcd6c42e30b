"""Every entry of the step kernel's 2x(9+3) Jacobian held to an extended-precision reference (tests/_jacref.py), each
within C E of it, E being the first-order running error bound of the kernel's own order of operations -- not one scale
per problem.  Families (tests/_jacref.py: family) in both modes (bal: the table prepared from the 9-vectors; state: from
cam15, the J_l columns at the device's to_vec) and both observation orders (camera-major, and permuted so that the
slow-camera path serves most lanes); the benchmark's own instance through the placed launch; Level 1 over several chunks.
Checked by tests/test_jacobian_reference.py on the CPU: the reference against mpmath, the bound against the restated
kernel and against one-line mutations of it."""
import argparse

import numpy as np
import pytest

import _jacref as J

pytestmark = pytest.mark.gpu

PER_CAM = 8                 # observations per camera: camera-major waves stage 8 cameras; permuted, every lane differs
M = 16_384                  # observations per family


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build()
    import torch
    import city2ba_amd
    from city2ba_amd import device as D
    assert city2ba_amd.device_count() > 0
    return dict(torch=torch, D=D, dev=torch.device("cuda", 0))


def _tables(env, mode, bal9):
    """(camblk, cams per camera for the restatement, to_vec per camera or None)"""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    b = torch.from_numpy(np.ascontiguousarray(bal9)).to(dev)
    if mode == "bal":
        return D.cameras_prepare_bal(b), bal9, None
    cam15 = D.cameras_from_bal(b)
    camblk = D.cameras_prepare_state(cam15)
    w = D.cameras_to_bal(cam15)[:, 0:3].contiguous()
    torch.cuda.synchronize()
    return camblk, cam15.cpu().numpy(), w.cpu().numpy()


def _launch(env, camblk, cam_of, X, order):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    n = len(order)
    pts4 = D.points_pad(torch.from_numpy(np.ascontiguousarray(X)).to(dev))
    ci = torch.from_numpy(cam_of[order].astype(np.int32)).to(dev)
    pi = torch.from_numpy(order.astype(np.int32)).to(dev)
    uv = torch.zeros((n, 2), dtype=torch.float64, device=dev)
    r = torch.empty((n, 2), dtype=torch.float64, device=dev)
    Jc = torch.full((n, 18), float("nan"), dtype=torch.float64, device=dev)
    Jp = torch.full((n, 6), float("nan"), dtype=torch.float64, device=dev)
    D.residual_jacobian(camblk, pts4, ci, pi, uv, r, Jc, Jp, 2.0, None)
    torch.cuda.synchronize()
    return Jc.cpu().numpy().reshape(n, 2, 9), Jp.cpu().numpy().reshape(n, 2, 3)


def _reference(mode, cams, w, X):
    if mode == "bal":
        return J.reference_bal(cams, X)
    return J.reference_state(cams, w, X)


def _check(label, Jc, Jp, ref, Ec, Ep):
    msg = (J.worst_report(Jc, ref["Jc"], Ec, J.COLS, label + " Jc") +
           J.worst_report(Jp, ref["Jp"], Ep, J.PCOLS, label + " Jp"))
    assert not msg, msg
    worst = max(J.ratio(Jc, ref["Jc"], Ec), J.ratio(Jp, ref["Jp"], Ep))
    print("[jacobian entries] %s: worst |err|/E = %.3g" % (label, worst))
    return worst


@pytest.mark.parametrize("mode", ["bal", "state"])
@pytest.mark.parametrize("fam", J.FAMILIES)
def test_families(env, fam, mode):
    bal9, cam_of, X, lab = J.family(fam, M, seed=101 + J.FAMILIES.index(fam), mode=mode, per_cam=PER_CAM)
    camblk, cams, w = _tables(env, mode, bal9)
    cams_o, w_o = cams[cam_of], (None if w is None else w[cam_of])
    ref = _reference(mode, cams_o, w_o, X)
    _, Ec, _, Ep = J.bounds(mode, cams_o, X, w_o)
    perm = np.random.default_rng(7).permutation(len(X))
    for order_name, order in (("camera-major", np.arange(len(X))), ("permuted", perm)):
        Jc, Jp = _launch(env, camblk, cam_of, X, order)
        inv = np.empty_like(order)
        inv[order] = np.arange(len(order))
        Jc, Jp = Jc[inv], Jp[inv]
        _check("%s/%s/%s" % (fam, mode, order_name), Jc, Jp, ref, Ec, Ep)
        if fam == "geometry":
            ax = lab == "axis"                           # p = 0 exactly: the f, k1, k2 and t2 columns are exactly zero
            assert ax.sum() > 100 and np.all(ref["Jc"][ax][:, :, 5:9] == 0)
            assert np.all(Jc[ax][:, :, 5:9] == 0), "%s/%s: a nonzero t2 / f / k1 / k2 entry on the optical axis" % (fam, mode)
    if fam == "angles":
        # every branch seen in both orders: per |w| label, the worst ratio
        for key in sorted(set(lab)):
            sel = lab == key
            print("[jacobian entries]   %s/%s %s: |err|/E = %.3g" % (fam, mode, key, J.ratio(Jc[sel], ref["Jc"][sel], Ec[sel])))


def test_state_tables_hold_the_restated_left_jacobian(env):
    """the J_l columns of a table prepared from cam15 are left_jacobian(to_vec) -- to_vec as cameras_to_bal reports it: bit
    for bit on the series branch (no transcendental in it), within C E on the other; R, t and intrinsics copied exactly"""
    D = env["D"]
    bal9, _, _, _ = J.family("angles", 64 * PER_CAM, seed=5, mode="state", per_cam=PER_CAM)
    camblk, cam15, w = _tables(env, "state", bal9)
    rec = D.camblk_records(camblk).cpu().numpy()
    Rrm = cam15[:, 0:9].reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9)
    assert np.array_equal(rec[:, 0:9].view(np.uint64), Rrm.view(np.uint64))
    assert np.array_equal(rec[:, 9:15].view(np.uint64), cam15[:, 9:15].view(np.uint64))
    Jl = J.left_jacobian(*(J.V(w[:, k]) for k in range(3)))
    got = rec[:, 15:24]
    want = np.stack([x.v for x in Jl], axis=1)
    E = np.stack([x.e for x in Jl], axis=1)
    series = ((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]) < 1e-2
    assert series.sum() > 10 and (~series).sum() > 10
    assert np.array_equal(got[series].view(np.uint64), want[series].view(np.uint64))
    ref = J.left_jacobian_ld(w).reshape(-1, 9)
    assert np.all(np.abs(got - ref).astype(np.float64) <= J.tolerance(E, ref))


def test_benchmark_instance(env):
    """synthetic --blocks 4 whole, and three 200k windows (start, middle, end) of --blocks 128, through the placed launch
    bench.py times (state mode: the generator's cameras, J_l at their to_vec)"""
    torch, D, dev = env["torch"], env["D"], env["dev"]
    import bench
    for blocks in (4, 128):
        sh = bench.build_shard(argparse.Namespace(blocks=blocks), 0, 1, dev)
        n = sh["n_obs"]
        outs = D.JacobianOutputs(n, dev, max_attempts=1)
        D.residual_jacobian_rows_placed(sh["camblk"], sh["pts4"], sh["rows"], sh["pt_idx"], sh["uv"], outs, 2.0)
        torch.cuda.synchronize()
        cam15 = sh["cam15"].cpu().numpy()
        w = D.cameras_to_bal(sh["cam15"])[:, 0:3].cpu().numpy()
        pts = sh["pts4"][:, 0:3].cpu().numpy()
        wins = [(0, n)] if blocks == 4 else [(0, 200_000), (n // 2 - 100_000, n // 2 + 100_000), (n - 200_000, n)]
        for lo, hi in wins:
            ci = sh["cam_idx"][lo:hi].cpu().numpy().astype(np.int64)
            pi = sh["pt_idx"][lo:hi].cpu().numpy().astype(np.int64)
            X = pts[pi]
            Jc = outs.Jc[lo:hi].cpu().numpy().reshape(-1, 2, 9)
            Jp = outs.Jp[lo:hi].cpu().numpy().reshape(-1, 2, 3)
            ref = J.reference_state(cam15[ci], w[ci], X)
            _, Ec, _, Ep = J.bounds("state", cam15[ci], X, w[ci])
            _check("synthetic --blocks %d [%d, %d)" % (blocks, lo, hi), Jc, Jp, ref, Ec, Ep)
        del outs, sh
        torch.cuda.empty_cache()


def test_level1_multi_chunk(env):
    """BAProblem.residual_jacobian() over 270 336 observations (more than one 256k chunk), bal mode"""
    import city2ba_amd
    bal9, cam_of, X, _ = J.family("pixel", 270_336, seed=77, mode="bal", per_cam=96)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam_of, minlength=len(bal9)))]).astype(np.uint64)
    pt_idx = np.arange(len(X), dtype=np.uint64)
    ba = city2ba_amd.BAProblem.from_bal(bal9, X, row_ptr, pt_idx, np.zeros((len(X), 2)))
    _, Jc, Jp = ba.residual_jacobian()
    ref = J.reference_bal(bal9[cam_of], X)
    _, Ec, _, Ep = J.bounds("bal", bal9[cam_of], X)
    _check("level 1 (bal, %d observations)" % len(X), Jc, Jp, ref, Ec, Ep)
