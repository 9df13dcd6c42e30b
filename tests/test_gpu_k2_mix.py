"""Waves that mix cameras with k2 == 0 and k2 != 0, in every per-observation kernel.

The light passes (k_observations: project, error sums, the L1 + L2 pair, observation noise + sums, visibility) project
every lane with |p|^4 = n * n, keep the lanes whose camera has k2 != 0 as a ballot mask, and rerun the tail with
libm's pow for those behind one wave-uniform branch; the slow-camera loop (unsorted input, more cameras in a wave than
the tile stages) patches that mask camera by camera and, for the lanes it served, reads the intrinsics from the table.
Taking the wrong route moves a pixel by about one ulp x k2, so the projections, residuals and visibility records are
held to the oracle BIT FOR BIT, and the error sums to exactly 0.0 where uv is the oracle's own projection.

The step kernel (k_residual_jacobian_l) runs its inlined pow route in every launch shape and stream policy, the shapes
of two tiles per wave and of 256-thread workgroups only above 6 M observations: one grid shard of that size with half
its cameras given k2 != 0 runs through all of them."""
import argparse
import functools

import numpy as np
import pytest

import oracle as O
from _problems import K2_PATTERNS, mixed_k2_cameras, points_in_front, random_problem, wave_first_cameras

pytestmark = pytest.mark.gpu

# every wave of these kernels opens on one of these observation counts: 3 tiles of 64 (the light passes), 1 or 2 (the
# step kernel); first_differs marks the camera that opens each of them
WAVE_OBS = (64, 128, 192)
LIST_SHAPES = ("ragged", "empties", "singles", "tile_edges", "ragged_tail")
ORDERS = ("camera_major", "permuted")
NORMS = (1.0, 2.0, 1.5)                        # 1.5: the NORM_ANY path with its pow table


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build()
    import torch
    import city2ba_amd
    from city2ba_amd import device as D
    assert city2ba_amd.device_count() > 0
    return dict(torch=torch, D=D, dev=torch.device("cuda", 0))


def _lists(kind, rng):
    if kind == "ragged":
        return rng.integers(1, 60, size=300)
    if kind == "empties":                      # empty lists at the start, inside tiles, in runs, at the end
        c = rng.integers(0, 50, size=400)
        c[rng.random(400) < 0.3] = 0
        c[:3] = 0
        c[-2:] = 0
        c[100:120] = 0
        return c
    if kind == "singles":                      # one observation per camera: 64 cameras per tile, more than are staged
        return np.ones(1000, dtype=np.int64)
    if kind == "tile_edges":                   # list boundaries exactly on multiples of 64 and 192
        return np.array([64, 64, 64, 128, 192, 1, 63, 191, 1, 0, 64])
    if kind == "ragged_tail":                  # short lists; the last wave's second tile holds one observation
        c = rng.integers(1, 9, size=500)
        c[-1] += (65 - int(c.sum())) % 192
        assert int(c.sum()) % 192 == 65
        return c
    raise AssertionError(kind)


@functools.lru_cache(maxsize=None)
def _case(pattern, kind, order):
    """host inputs and the oracle's answers, camera-major; `idx` puts them into launch order"""
    seed = sum(f"{pattern}/{kind}".encode())
    rng = np.random.default_rng(seed)
    counts = np.asarray(_lists(kind, rng), dtype=np.int64)
    n_cam, n = len(counts), int(counts.sum())
    cam_of = np.repeat(np.arange(n_cam), counts)
    idx = np.arange(n) if order == "camera_major" else rng.permutation(n)
    # rotation angles below 0.05 raised to 0.05: there the oracle's closed-form Jacobian in w loses ~eps / |w|^2 of relative
    # precision (at |w| = 4e-4 it is 4e-8 off an mpmath derivative where the kernel is 7e-10 off), more than the 1e-10
    # the kernel is held to here
    bal9 = random_problem(n_cam, 1, 0, seed=seed)["bal9"].copy()
    w = np.linalg.norm(bal9[:, :3], axis=1, keepdims=True)
    bal9[:, :3] *= np.where(w < 0.05, 0.05 / w, 1.0)
    cams = mixed_k2_cameras(O.camera_from_bal(bal9), pattern, seed, firsts=wave_first_cameras(cam_of[idx], WAVE_OBS))
    k2 = cams[:, 14]
    assert (k2[cam_of] == 0.0).any() and (k2[cam_of] != 0.0).any()
    pts = points_in_front(cams, cam_of, seed)  # point j is observation j's
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    pt = np.arange(n, dtype=np.uint64)
    proj = O.project_observations(cams, pts, row_ptr, pt)
    assert np.isfinite(proj).all()
    uv_noisy = proj + rng.normal(scale=1e-3, size=proj.shape)
    r0, Jc0, Jp0 = O.residual_jacobian(cams, pts, row_ptr, pt, uv_noisy)
    sums = {norm: O.reprojection_error_sum(cams, pts, row_ptr, pt, uv_noisy, norm) for norm in NORMS}
    # visibility: each camera sees the points of others (behind it, in front, inside or outside the frame); max_dist
    # at the median distance, so that both sides of it occur
    pt_vis = rng.permutation(n).astype(np.int64)
    d = np.linalg.norm(O.centers(cams)[cam_of] - pts[pt_vis], axis=1)
    max_dist = float(np.median(d))
    vis_uv, keep = O.visibility_pairs(cams, pts, cam_of, pt_vis, max_dist)
    if n > 500:
        front = ~np.isnan(vis_uv[:, 0])
        assert keep.any() and (front & ~keep.astype(bool)).any() and (~front).any()
    return dict(n=n, n_cam=n_cam, counts=counts, cam_of=cam_of, idx=idx, cams=cams, pts=pts, row_ptr=row_ptr, proj=proj,
                uv_noisy=uv_noisy, r0=r0, Jc0=Jc0, Jp0=Jp0, sums=sums, pt_vis=pt_vis, max_dist=max_dist, vis_uv=vis_uv,
                keep=keep)


def _device(env, c):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    i = c["idx"]
    rp = np.concatenate([[0], np.cumsum(c["counts"])]).astype(np.int64)
    return dict(camblk=D.cameras_prepare_state(t(c["cams"])), pts4=D.points_pad(t(c["pts"])),
                ci=t(c["cam_of"][i].astype(np.int32)), pi=t(i.astype(np.int32)), pi_vis=t(c["pt_vis"][i].astype(np.int32)),
                uv_exact=t(c["proj"][i]), uv_noisy=t(c["uv_noisy"][i]), rows=D.Rows(t(rp)), ws=D.workspace(c["n"], dev))


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", LIST_SHAPES)
@pytest.mark.parametrize("pattern", K2_PATTERNS)
def test_light_passes_bit_exact_on_mixed_k2_waves(env, pattern, kind, order):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    c = _case(pattern, kind, order)
    g = _device(env, c)
    n, i = c["n"], c["idx"]
    cb, p4, ws = g["camblk"], g["pts4"], g["ws"]
    zero = lambda k=1: torch.full((k,), -1.0, dtype=torch.float64, device=dev)
    full = lambda: torch.full((n, 2), 7.0, dtype=torch.float64, device=dev)

    # projection
    a = full()
    D.project(cb, p4, g["ci"], g["pi"], a)
    torch.cuda.synchronize()
    assert _same_bits(a, c["proj"][i])

    # visibility: uv (NaN where the point is behind the camera or too far) and keep
    keep = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    D.visibility_pairs(cb, p4, g["ci"], g["pi_vis"], c["max_dist"], a, keep)
    torch.cuda.synchronize()
    assert _same_bits(a, c["vis_uv"][i]) and np.array_equal(keep.cpu().numpy(), c["keep"][i])

    # error sums: exactly zero against the exact projection; the oracle's to rounding against a noisy one
    for norm in NORMS:
        e = zero()
        D.reprojection_error_sum(cb, p4, g["ci"], g["pi"], g["uv_exact"], norm, ws, e)
        torch.cuda.synchronize()
        assert e.item() == 0.0, norm
        D.reprojection_error_sum(cb, p4, g["ci"], g["pi"], g["uv_noisy"], norm, ws, e)
        torch.cuda.synchronize()
        assert abs(e.item() - c["sums"][norm]) <= 1e-12 * c["sums"][norm], norm

    if order != "camera_major":
        return
    rows, pi = g["rows"], g["pi"]
    b = full()
    D.project_rows(cb, p4, rows, pi, b)
    torch.cuda.synchronize()
    assert _same_bits(b, c["proj"])

    # the row-structure visibility, byte keep and bit keep
    pt_vis = torch.from_numpy(c["pt_vis"].astype(np.int32)).to(dev)
    keep.fill_(9)
    D.visibility_rows(cb, p4, rows, pt_vis, c["max_dist"], b, keep)
    words = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=dev)
    b2 = full()
    D.visibility_rows_bits(cb, p4, rows, pt_vis, c["max_dist"], b2, words)
    torch.cuda.synchronize()
    assert _same_bits(b, c["vis_uv"]) and np.array_equal(keep.cpu().numpy(), c["keep"])
    bits = np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")
    assert _same_bits(b2, c["vis_uv"]) and np.array_equal(bits[:n], c["keep"]) and not bits[n:].any()

    for norm in NORMS:
        e = zero()
        D.reprojection_error_sum_rows(cb, p4, rows, pi, g["uv_exact"], norm, ws, e)
        torch.cuda.synchronize()
        assert e.item() == 0.0, norm
        D.reprojection_error_sum_rows(cb, p4, rows, pi, g["uv_noisy"], norm, ws, e)
        torch.cuda.synchronize()
        assert abs(e.item() - c["sums"][norm]) <= 1e-12 * c["sums"][norm], norm
    both = zero(2)
    D.reprojection_error_sums2_rows(cb, p4, rows, pi, g["uv_exact"], ws, both)
    torch.cuda.synchronize()
    assert both.tolist() == [0.0, 0.0]
    D.reprojection_error_sums2_rows(cb, p4, rows, pi, g["uv_noisy"], ws, both)
    torch.cuda.synchronize()
    for k, norm in enumerate((1.0, 2.0)):
        assert abs(both[k].item() - c["sums"][norm]) <= 1e-12 * c["sums"][norm], norm

    # observation noise fused with the sums: at std 0 nothing moves and both sums are zero; at std > 0 the bits of
    # add_noise_observations followed by the L1 + L2 pass
    uv = g["uv_exact"].clone()
    D.add_noise_observations_error_sums2_rows(cb, p4, rows, pi, uv, 0, 0.0, 31, ws, both)
    torch.cuda.synchronize()
    assert both.tolist() == [0.0, 0.0] and _same_bits(uv, c["proj"])
    uv_a, uv_b = g["uv_exact"].clone(), g["uv_exact"].clone()
    want, got = zero(2), zero(2)
    D.add_noise_observations(uv_a, 0, 1e-3, 31)
    D.reprojection_error_sums2_rows(cb, p4, rows, pi, uv_a, ws, want)
    D.add_noise_observations_error_sums2_rows(cb, p4, rows, pi, uv_b, 0, 1e-3, 31, ws, got)
    torch.cuda.synchronize()
    assert _same_bits(uv_a, uv_b) and _same_bits(got, want) and want[1].item() > 0.0


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", LIST_SHAPES)
@pytest.mark.parametrize("pattern", K2_PATTERNS)
def test_step_kernel_on_mixed_k2_waves(env, pattern, kind, order):
    torch, D, dev = env["torch"], env["D"], env["dev"]
    c = _case(pattern, kind, order)
    g = _device(env, c)
    n, i = c["n"], c["idx"]
    cb, p4, ws = g["camblk"], g["pts4"], g["ws"]
    scale = max(1.0, float(np.max(np.abs(c["Jc0"]))))
    r_want = c["proj"] - c["uv_noisy"]
    outs = lambda: [torch.full((n, w), 5.0, dtype=torch.float64, device=dev) for w in (2, 18, 6)]

    def check(r, Jc, Jp, sel):
        assert _same_bits(r, r_want[sel])
        assert np.max(np.abs(Jc.cpu().numpy() - c["Jc0"][sel])) / scale < 1e-10
        assert np.max(np.abs(Jp.cpu().numpy() - c["Jp0"][sel])) / scale < 1e-10

    o = outs()
    D.residual_jacobian(cb, p4, g["ci"], g["pi"], g["uv_noisy"], *o, 2.0, None)
    torch.cuda.synchronize()
    check(*o, i)
    e = torch.full((1,), -1.0, dtype=torch.float64, device=dev)
    o2 = outs()
    D.residual_jacobian_sum(cb, p4, g["ci"], g["pi"], g["uv_exact"], *o2, 2.0, ws, e)
    torch.cuda.synchronize()
    assert e.item() == 0.0 and not o2[0].any()
    if order != "camera_major":
        return
    o3 = outs()
    D.residual_jacobian_rows(cb, p4, g["rows"], g["pi"], g["uv_noisy"], *o3, 2.0, None)
    torch.cuda.synchronize()
    check(*o3, i)
    for w in range(3):
        assert torch.equal(o3[w].view(torch.int64), o[w].view(torch.int64))
    e.fill_(-1.0)
    D.residual_jacobian_rows(cb, p4, g["rows"], g["pi"], g["uv_exact"], *o3, 2.0, ws, e)
    torch.cuda.synchronize()
    assert e.item() == 0.0 and not o3[0].any()


def test_level1_problem_with_mixed_k2(env):
    import city2ba_amd as c2b
    P = random_problem(260, 3000, 14, seed=314)
    cams = mixed_k2_cameras(P["cams15"], "signs", seed=9)
    uv = O.project_observations(cams, P["pts"], P["row_ptr"], P["pt_idx"])
    uv = uv + np.random.default_rng(2).normal(scale=1e-3, size=uv.shape)
    ba = c2b.BAProblem.from_visibility(cams, P["pts"], P["row_ptr"], P["pt_idx"], uv, device=0)
    assert _same_bits(ba.project(), O.project_observations(cams, P["pts"], P["row_ptr"], P["pt_idx"]))
    for norm in (1.0, 2.0):
        want = O.total_reprojection_error(cams, P["pts"], P["row_ptr"], P["pt_idx"], uv, norm)
        assert abs(ba.total_reprojection_error(norm) - want) <= 1e-12 * want
    ba.close()


def test_step_kernel_above_six_million_observations_with_k2(env):
    """synthetic --blocks 72: 6 132 074 observations, just past the size where the step kernel's launches take two tiles
    per wave (and 256-thread workgroups into a slow-store set).  Half its cameras get k2 != 0; every launch shape, every
    stream policy and the unsorted cam_idx form write the same r / Jc / Jp bits, r is the oracle's projection minus uv
    bit for bit on the whole list, and Jc / Jp match the oracle on three windows."""
    import bench
    from city2ba_amd import _lib as L
    torch, D, dev = env["torch"], env["D"], env["dev"]
    sh = bench.build_shard(argparse.Namespace(blocks=72), 0, 1, dev)
    n, rows, pts4, pi = sh["n_obs"], sh["rows"], sh["pts4"], sh["pt_idx"]
    assert n == 6_132_074                      # the generator is deterministic: just past 6 M
    assert D.jacobian_tiles_per_wave(n) == 2
    cams = mixed_k2_cameras(sh["cam15"].cpu().numpy(), "half", seed=72)
    assert 0.4 < float(np.mean(cams[:, 14] != 0.0)) < 0.6
    camblk = D.cameras_prepare_state(torch.from_numpy(cams).to(dev))
    uv = torch.empty((n, 2), dtype=torch.float64, device=dev)
    D.project_rows(camblk, pts4, rows, pi, uv)
    D.add_noise_observations(uv, 0, 1e-3, 72)
    ws = D.workspace(n, dev)

    r = torch.full((n, 2), float("nan"), dtype=torch.float64, device=dev)
    Jc = torch.full((n, 18), float("nan"), dtype=torch.float64, device=dev)
    Jp = torch.full((n, 6), float("nan"), dtype=torch.float64, device=dev)
    e_ref = torch.zeros(1, dtype=torch.float64, device=dev)
    D.residual_jacobian_rows(camblk, pts4, rows, pi, uv, r, Jc, Jp, 2.0, ws, e_ref)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Jc).all()) and bool(torch.isfinite(Jp).all()) and e_ref.item() > 0.0

    def same(outs_r, outs_Jc, outs_Jp):
        return torch.equal(outs_r, r) and torch.equal(outs_Jc, Jc) and torch.equal(outs_Jp, Jp)

    # every launch shape (chosen by the placed set's store rate), each reproducing its own sum
    outs = D.JacobianOutputs(n, dev, max_attempts=1)
    e = torch.zeros(1, dtype=torch.float64, device=dev)
    shapes = {}
    for rate in (5700.0, 6500.0, 7100.0, 0.0):
        outs.set_store_rate(rate)
        shapes[rate] = D.jacobian_launch_shape(n, rate)
        sums = set()
        for _ in range(2):
            outs.r.fill_(float("nan")); outs.Jc.fill_(float("nan")); outs.Jp.fill_(float("nan"))
            D.residual_jacobian_rows_placed(camblk, pts4, rows, pi, uv, outs, 2.0, ws, e)
            torch.cuda.synchronize()
            sums.add(e.item())
            assert same(outs.r, outs.Jc, outs.Jp), rate
        assert len(sums) == 1 and abs(e.item() - e_ref.item()) <= 1e-13 * e_ref.item()
    assert shapes == {5700.0: (4, 1), 6500.0: (16, 1), 7100.0: (8, 2), 0.0: (8, 2)}

    # every stream policy (n_pts only sizes the cache-policy choice)
    lib, p = L.lib(), (lambda t: t.data_ptr())
    for want in (0, 2, 3):
        fake = next(k for k in [pts4.shape[0]] + list(range(100_000, 8_000_000, 50_000))
                    if lib.c2b_jacobian_stream_policy(n, rows.n_cam, k) == want)
        outs.r.fill_(float("nan")); outs.Jc.fill_(float("nan")); outs.Jp.fill_(float("nan")); e.fill_(-1.0)
        assert lib.c2b_residual_jacobian_rows(p(camblk), p(pts4), fake, p(rows.row_ptr), rows.n_cam, p(rows.tiles), 0, p(pi),
                                              p(uv), n, p(outs.r), p(outs.Jc), p(outs.Jp), 2.0, p(ws), p(e), None) == L.OK
        torch.cuda.synchronize()
        assert e.item() == e_ref.item() and same(outs.r, outs.Jc, outs.Jp), want

    # the cam_idx form on a random permutation: the two-tile instance's slow-camera loop on every lane
    perm = torch.from_numpy(np.random.default_rng(72).permutation(n)).to(dev)
    D.residual_jacobian(camblk, pts4, sh["cam_idx"][perm].contiguous(), pi[perm].contiguous(), uv[perm].contiguous(),
                        outs.r, outs.Jc, outs.Jp, 2.0, None)
    torch.cuda.synchronize()
    assert torch.equal(outs.r, r[perm]) and torch.equal(outs.Jc, Jc[perm]) and torch.equal(outs.Jp, Jp[perm])
    del outs, perm

    # the oracle: r bit for bit on the whole list, Jc / Jp on three windows
    pts = np.ascontiguousarray(pts4[:, :3].cpu().numpy())
    row_ptr = rows.row_ptr.cpu().numpy().astype(np.uint64)
    pi_h = pi.cpu().numpy().astype(np.uint64)
    uv_h = uv.cpu().numpy()
    r_h = r.cpu().numpy()
    assert _same_bits(r_h, O.project_observations(cams, pts, row_ptr, pi_h) - uv_h)
    ci_h = sh["cam_idx"].cpu().numpy().astype(np.int64)
    for lo in (0, n // 2, n - 20_000):
        hi = lo + 20_000
        c0, c1 = int(ci_h[lo]), int(ci_h[hi - 1]) + 1
        counts = np.bincount(ci_h[lo:hi] - c0, minlength=c1 - c0)
        rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        r0, Jc0, Jp0 = O.residual_jacobian(cams[c0:c1], pts, rp, pi_h[lo:hi], uv_h[lo:hi])
        assert _same_bits(r_h[lo:hi], r0)
        scale = max(1.0, float(np.max(np.abs(Jc0))))
        assert np.max(np.abs(Jc[lo:hi].cpu().numpy() - Jc0)) / scale < 1e-10
        assert np.max(np.abs(Jp[lo:hi].cpu().numpy() - Jp0)) / scale < 1e-10
    del r, Jc, Jp, uv, ws, camblk, sh
    torch.cuda.empty_cache()
