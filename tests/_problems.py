"""Seeded synthetic BA problems shared by the CPU and GPU tests (inputs only)."""
import math

import numpy as np

import oracle as O


def random_problem(n_cam, n_pts, obs_per_cam, seed, noise=0.0, k_scale=1e-2, empty_every=0):
    """Cameras with w in (-pi,pi)^3-ish, every observed point in front of its camera.

    Returns dict(bal9, cams15, pts, row_ptr(u64), pt_idx(u64), uv) with uv = exact oracle
    projection (+ optional gaussian noise)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-np.pi, np.pi, size=(n_cam, 3)) * rng.uniform(0.0, 1.0, size=(n_cam, 1))
    t = rng.uniform(-50, 50, size=(n_cam, 3))
    intr = np.column_stack([rng.uniform(0.8, 1.2, n_cam), rng.uniform(-k_scale, k_scale, n_cam),
                            rng.uniform(-k_scale, k_scale, n_cam)])
    bal9 = np.ascontiguousarray(np.column_stack([w, t, intr]))
    cams15 = O.camera_from_bal(bal9)
    pts = np.empty((n_pts, 3))
    row_ptr = [0]
    pt_idx = []
    owner = rng.integers(0, n_cam, size=n_pts)          # each point placed in front of one camera
    for j in range(n_pts):
        z = -rng.uniform(1.0, 10.0)
        q = np.array([rng.uniform(-0.9, 0.9) * -z, rng.uniform(-0.9, 0.9) * -z, z])
        pts[j] = O.to_world(cams15[owner[j]], q)
    by_owner = [np.nonzero(owner == c)[0] for c in range(n_cam)]
    for c in range(n_cam):
        if empty_every and c % empty_every == 0:
            row_ptr.append(len(pt_idx)); continue
        mine = by_owner[c]
        k = min(obs_per_cam, len(mine))
        pick = rng.choice(mine, size=k, replace=False) if k else np.empty(0, dtype=int)
        pt_idx.extend(int(x) for x in pick)
        row_ptr.append(len(pt_idx))
    row_ptr = np.asarray(row_ptr, dtype=np.uint64)
    pt_idx = np.asarray(pt_idx, dtype=np.uint64)
    uv = O.project_observations(cams15, pts, row_ptr, pt_idx)
    if noise:
        uv = uv + rng.normal(scale=noise, size=uv.shape)
    return dict(bal9=bal9, cams15=cams15, pts=pts, row_ptr=row_ptr, pt_idx=pt_idx, uv=uv)


def grid_cameras_points(num_blocks, cpb=10, ppb=10, L=20.0, inset=1.0, cam_h=1.0, pt_h=1.0):
    """Camera / point layout of src/synthetic.rs:178-258 (layout only; visibility is computed by
    the caller).  Returns cams15 (via the oracle's from_position_direction) and pts."""
    dirs = {"-90": O.basis_from_angle_y_deg(-90.0), "90": O.basis_from_angle_y_deg(90.0),
            "180": O.basis_from_angle_y_deg(180.0), "one": np.array([1, 0, 0, 0, 1, 0, 0, 0, 1.0])}
    cams, pts = [], []
    for bx in range(num_blocks + 1):
        ox = L * bx
        for by in range(num_blocks + 1):
            oz = L * by
            for i in range(cpb):
                if bx != num_blocks:
                    loc = [ox + i / cpb * L, cam_h, oz]
                    cams.append(O.from_position_direction(loc, dirs["-90"]))
                    cams.append(O.from_position_direction(loc, dirs["90"]))
                if by != num_blocks:
                    loc = [ox, cam_h, oz + i / cpb * L]
                    cams.append(O.from_position_direction(loc, dirs["180"]))
                    cams.append(O.from_position_direction(loc, dirs["one"]))
    for bx in range(num_blocks + 1):
        ox = L * bx
        for by in range(num_blocks + 1):
            oz = L * by
            for i in range(ppb):
                step = (L - inset * 2.0) / ppb
                if bx != num_blocks:
                    lx = ox + inset + i * step
                    pts += [[lx, pt_h, oz - inset], [lx, pt_h, oz + inset],
                            [lx + step / 2.0, 0.0, oz - inset], [lx + step / 2.0, 0.0, oz + inset],
                            [lx + step / 2.0, 0.0, oz - inset / 2.0], [lx + step / 2.0, 0.0, oz + inset / 2.0]]
                if by != num_blocks:
                    lz = oz + inset + i * step
                    pts += [[ox - inset, pt_h, lz], [ox + inset, pt_h, lz],
                            [ox - inset, 0.0, lz + step / 2.0], [ox + inset, 0.0, lz + step / 2.0],
                            [ox - inset / 2.0, 0.0, lz + step / 2.0], [ox + inset / 2.0, 0.0, lz + step / 2.0]]
    return np.asarray(cams), np.asarray(pts, dtype=np.float64)


def grid_candidate_pairs(cams15, pts, max_dist):
    """All (camera, point) pairs with |center - p|^2 <= max_dist^2, camera-major, point index
    ascending (a canonical order; rstar's traversal order is not reproducible)."""
    ctr = O.centers(cams15)
    cam_idx, pt_idx = [], []
    for c in range(len(cams15)):
        d2 = ((pts - ctr[c]) ** 2).sum(axis=1)
        sel = np.nonzero(d2 <= max_dist * max_dist)[0]
        cam_idx.append(np.full(len(sel), c, dtype=np.uint32))
        pt_idx.append(sel.astype(np.uint32))
    return np.concatenate(cam_idx), np.concatenate(pt_idx)


# ---- numpy restatement of the grid layout / candidate search (independent of the C++ host code) ----
def _basis_y(deg):
    """Basis3::from_angle_y(Deg(deg)) as col-major 9 (cgmath: Deg -> Rad is deg * (PI/180));
    libm sin/cos like Rust's f64::sin_cos."""
    th = deg * (math.pi / 180.0)
    s, c = math.sin(th), math.cos(th)
    return np.array([c, 0.0, -s, 0.0, 1.0, 0.0, s, 0.0, c])


def np_grid_layout(num_blocks, cpb=10, ppb=10, block_length=20.0, block_inset=1.0, camera_height=1.0,
                point_height=1.0):
    """cams15 [4*cpb*B*(B+1), 15] and pts [12*ppb*B*(B+1), 3] in the reference's push order."""
    B, L, ins = int(num_blocks), float(block_length), float(block_inset)
    assert ins * 2.0 < L, "Block inset must be less than half the block length"
    bx, by, i, k = np.meshgrid(np.arange(B + 1), np.arange(B + 1), np.arange(cpb), np.arange(4), indexing="ij")
    bx, by, i, k = bx.ravel(), by.ravel(), i.ravel(), k.ravel()
    horiz = k < 2
    ok = np.where(horiz, bx != B, by != B)
    bx, by, i, k, horiz = bx[ok], by[ok], i[ok], k[ok], horiz[ok]
    off_x, off_z = L * bx.astype(np.float64), L * by.astype(np.float64)
    along = i.astype(np.float64) / float(cpb) * L
    px = np.where(horiz, off_x + along, off_x)
    pz = np.where(horiz, off_z, off_z + along)
    py = np.full_like(px, float(camera_height))
    dirs = np.stack([_basis_y(-90.0), _basis_y(90.0), _basis_y(180.0), np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1])])
    R = dirs[k]                                               # [n, 9] col-major
    # from_position_direction (src/baproblem.rs:153-159): loc = -1.0 * (dir . pos), dot = (a+b)+c
    t = np.stack([-1.0 * ((R[:, 0] * px + R[:, 3] * py) + R[:, 6] * pz),
                  -1.0 * ((R[:, 1] * px + R[:, 4] * py) + R[:, 7] * pz),
                  -1.0 * ((R[:, 2] * px + R[:, 5] * py) + R[:, 8] * pz)], axis=1)
    intr = np.tile(np.array([1.0, 0.0, 0.0]), (len(px), 1))
    cams15 = np.ascontiguousarray(np.concatenate([R, t, intr], axis=1))

    step = (L - ins * 2.0) / float(ppb)
    bx, by, i, k = np.meshgrid(np.arange(B + 1), np.arange(B + 1), np.arange(ppb), np.arange(12), indexing="ij")
    bx, by, i, k = bx.ravel(), by.ravel(), i.ravel(), k.ravel()
    horiz = k < 6
    ok = np.where(horiz, bx != B, by != B)
    bx, by, i, k, horiz = bx[ok], by[ok], i[ok], k[ok], horiz[ok]
    off_x, off_z = L * bx.astype(np.float64), L * by.astype(np.float64)
    kk = k % 6
    base = np.where(horiz, off_x, off_z) + ins + i.astype(np.float64) * step     # loc_x / loc_z
    along = np.where(kk < 2, base, base + step / 2.0)
    other0 = np.where(horiz, off_z, off_x)
    lateral = np.select([kk == 0, kk == 1, kk == 2, kk == 3, kk == 4, kk == 5],
                        [other0 - ins, other0 + ins, other0 - ins, other0 + ins,
                         other0 - ins / 2.0, other0 + ins / 2.0])
    y = np.where(kk < 2, float(point_height), 0.0)
    x = np.where(horiz, along, lateral)
    z = np.where(horiz, lateral, along)
    pts = np.ascontiguousarray(np.stack([x, y, z], axis=1))
    return cams15, pts


def np_candidate_pairs(centers, pts, max_dist, cam_lo=0, cam_hi=None, chunk=100_000):
    """(cam, point) pairs with |center - p|^2 <= max_dist^2 (rstar's locate_within_distance takes the
    squared radius, src/synthetic.rs:277-280), camera-major, ascending point index per camera.
    Uniform-cell binning over (x, z)."""
    cam_hi = len(centers) if cam_hi is None else cam_hi
    cs = float(max_dist)
    x0 = min(pts[:, 0].min(), centers[:, 0].min()) - cs
    z0 = min(pts[:, 2].min(), centers[:, 2].min()) - cs
    pcx = np.floor((pts[:, 0] - x0) / cs).astype(np.int64)
    pcz = np.floor((pts[:, 2] - z0) / cs).astype(np.int64)
    ncz = int(pcz.max()) + 3
    ncx = int(pcx.max()) + 3
    cell = pcx * ncz + pcz
    order = np.argsort(cell, kind="stable")
    sorted_cell = cell[order]
    starts = np.searchsorted(sorted_cell, np.arange(ncx * ncz + 1))
    out_c, out_p = [], []
    r2 = max_dist * max_dist
    for lo in range(cam_lo, cam_hi, chunk):
        hi = min(lo + chunk, cam_hi)
        c = centers[lo:hi]
        ccx = np.floor((c[:, 0] - x0) / cs).astype(np.int64)
        ccz = np.floor((c[:, 2] - z0) / cs).astype(np.int64)
        cams, pidx = [], []
        for dx in (-1, 0, 1):
            for dz in (-1, 0, 1):
                cid = (ccx + dx) * ncz + (ccz + dz)
                s, e = starts[cid], starts[cid + 1]
                ln = e - s
                tot = int(ln.sum())
                if tot == 0:
                    continue
                rep = np.repeat(np.arange(lo, hi), ln)
                first = np.repeat(np.cumsum(ln) - ln, ln)
                pos = np.arange(tot) - first + np.repeat(s, ln)
                cams.append(rep)
                pidx.append(order[pos])
        cams = np.concatenate(cams)
        pidx = np.concatenate(pidx)
        d = pts[pidx] - centers[cams]
        keep = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r2
        cams, pidx = cams[keep], pidx[keep]
        o = np.lexsort((pidx, cams))
        out_c.append(cams[o].astype(np.int32))
        out_p.append(pidx[o].astype(np.int32))
    if not out_c:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    return np.concatenate(out_c), np.concatenate(out_p)


# ---- cameras whose radial term k2 differs from camera to camera (some 0, some not) ----
K2_PATTERNS = ("half", "alternate", "lone", "signs", "first_differs")


def wave_first_cameras(cam_of, wave_obs):
    """Cameras of the observations that open a wave, for waves of each length in `wave_obs` observations, read off the
    observation list in launch order (cam_of[i] = camera of observation i)."""
    cam_of = np.asarray(cam_of)
    firsts = set()
    for w in wave_obs:
        firsts.update(int(c) for c in cam_of[::int(w)])
    return np.array(sorted(firsts), dtype=np.int64)


def mixed_k2_cameras(cams15, pattern, seed, firsts=None):
    """A copy of cams15 with k2 (column 14) rewritten camera by camera, so that waves mix cameras with k2 == 0 and
    k2 != 0:
      half           nonzero with probability 1/2;
      alternate      odd cameras nonzero, even ones zero;
      lone           first half of the cameras: one in 13 nonzero; second half: one in 13 zero;
      signs          in turn 0.0, -0.0, the smallest subnormal 5e-324 (either sign), |k2| around 1 and around 1e-2, both
                     signs;
      first_differs  the cameras in `firsts` (wave_first_cameras) nonzero, every other camera zero."""
    rng = np.random.default_rng(seed)
    n = len(cams15)
    c = np.arange(n)
    small = rng.uniform(-1e-2, 1e-2, n)
    if pattern == "half":
        k2 = np.where(rng.random(n) < 0.5, small, 0.0)
    elif pattern == "alternate":
        k2 = np.where(c % 2 == 1, small, 0.0)
    elif pattern == "lone":
        k2 = np.where((c < n // 2) == (c % 13 == 0), small, 0.0)
    elif pattern == "signs":
        choices = np.array([0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, 1e-2, -1e-2])
        k2 = choices[c % len(choices)]
        k2 = np.where(np.abs(k2) >= 1e-2, k2 * rng.uniform(0.5, 1.5, n), k2)
    elif pattern == "first_differs":
        assert firsts is not None
        k2 = np.zeros(n)
        k2[firsts] = np.where(small[firsts] != 0.0, small[firsts], 1e-3)
    else:
        raise AssertionError(pattern)
    out = np.array(cams15, dtype=np.float64, copy=True)
    out[:, 14] = k2
    return out


def points_in_front(cams15, cam_of, seed):
    """One world point per observation, in front of that observation's camera: camera-frame q with q.z in [-10, -1]
    and |q.x|, |q.y| <= 0.9 |q.z| (so |p| <= 1.3 and every projection and Jacobian stays of order one)."""
    rng = np.random.default_rng(seed)
    cam_of = np.asarray(cam_of, dtype=np.int64)
    m = len(cam_of)
    z = -rng.uniform(1.0, 10.0, m)
    q = np.stack([rng.uniform(-0.9, 0.9, m) * -z, rng.uniform(-0.9, 0.9, m) * -z, z], axis=1)
    M = cams15[cam_of, :9].reshape(m, 3, 3).transpose(0, 2, 1)       # R is column-major: q = R X + t
    X = np.linalg.solve(M, (q - cams15[cam_of, 9:12])[:, :, None])[:, :, 0]
    return np.ascontiguousarray(X)


# ---- a coupled general-position problem: shared points, general rotations, mixed distortion, chosen row lengths ----
# camera rows of these lengths: around the 16 lanes a camera gets in k_normal_cameras / k_schur_cameras / k_schur_jacobi
# and their multiples, an empty row, and rows of several hundred
DOME_LENGTHS = (0, 1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 130, 257)
DOME_N_CAM = 81                                                  # the 23 above + 58 drawn in 1..40; 81 % 4 == 1
DOME_N_PTS = 400
DOME_UNOBSERVED = 20                                             # the last points: no observation
DOME_SINGLES = 40                                                # points 1 .. 40: seen exactly once
DOME_CROWDED = 0                                                 # point 0: in every non-empty row


def _dome_rows(rng, dup):
    """(lengths, rows): the shuffled row lengths and each camera's point list.  Every non-empty row holds the crowded
    point; the singles go one each to rows of length >= 3; the rest is drawn without repeats from the shared points.
    Every third camera with at least 4 observations has one (camera, point) pair twice, at least two places apart -- the
    crowded point's in every other such camera; with dup = False that place holds one more distinct shared point, so both
    variants have the same lengths."""
    lengths = np.array(list(DOME_LENGTHS) + [int(v) for v in rng.integers(1, 41, DOME_N_CAM - len(DOME_LENGTHS))])
    rng.shuffle(lengths)
    shared = np.arange(DOME_SINGLES + 1, DOME_N_PTS - DOME_UNOBSERVED)
    takers = np.flatnonzero(lengths >= 3)
    single_of = {}
    for k, p in enumerate(range(1, DOME_SINGLES + 1)):
        single_of.setdefault(int(takers[k % len(takers)]), []).append(p)
    rows, n_dup_cams = [], 0
    for c, n in enumerate(lengths):
        n = int(n)
        if n == 0:
            rows.append(np.empty(0, dtype=np.int64))
            continue
        twice = n >= 4 and c % 3 == 0
        own = single_of.get(c, [])[:max(0, n - 2)]
        fill = rng.choice(shared, size=n - 1 - len(own) - (1 if twice else 0), replace=False)
        row = np.concatenate([[DOME_CROWDED], own, fill]).astype(np.int64)
        rng.shuffle(row)
        if twice:
            i = int(rng.integers(0, len(row)))
            if n_dup_cams % 2 == 0:
                i = int(np.flatnonzero(row == DOME_CROWDED)[0])
            elif row[i] <= DOME_SINGLES:                         # a shared point, so that the singles stay seen once
                i = int(np.flatnonzero(row > DOME_SINGLES)[0])
            far = [j for j in range(len(row) + 1) if j < i - 1 or j > i + 2]       # insert position: >= 2 places from i
            j = int(rng.choice(far))
            extra = row[i] if dup else rng.choice(np.setdiff1d(shared, row))
            row = np.insert(row, j, extra)
            n_dup_cams += 1
        assert len(row) == n
        rows.append(row)
    return lengths, rows


def dome_problem(seed=0, dup=True, state=False, obs_noise=1e-3, start_noise=1e-3):
    """DOME_N_CAM cameras on a shell of radius 8-14 around DOME_N_PTS points in the box [-2, 2]^3, each looking down its
    -z axis at a target within 0.5 of the origin with a random roll (every point is in front of every camera, |uv| up to
    about 0.5); the rotation vector is the oracle's to_rodrigues of the rotation matrix (angle 2 acos(q0): here 0.7 to 4.1); f in [0.8, 1.2], k1
    and k2 in +-5e-2, k2 = 0 on every fifth camera.  Rows: _dome_rows.  Observations are the oracle's projection of that
    state + obs_noise; the state returned is moved by start_noise in pose (w, t) and in the points.
    Returns dict(bal9, cams15 (= camera_from_bal(bal9)), pts, row_ptr (u64), pt_idx (u64), uv, lengths, true_bal9,
    true_pts, bal (= not state): load it with from_bal(bal9, ...) when bal, with from_visibility(cams15, ...) otherwise)."""
    rng = np.random.default_rng(seed)
    lengths, rows = _dome_rows(rng, dup)
    pts = rng.uniform(-2.0, 2.0, size=(DOME_N_PTS, 3))
    cams = np.empty((DOME_N_CAM, 15))
    for c in range(DOME_N_CAM):
        d = rng.normal(size=3)
        ctr = d / np.linalg.norm(d) * rng.uniform(8.0, 14.0)
        t = rng.normal(size=3)
        target = t / np.linalg.norm(t) * rng.uniform(0.0, 0.5)
        z = (ctr - target) / np.linalg.norm(ctr - target)        # the camera looks down -z
        a = np.cross(z, rng.normal(size=3))
        x = a / np.linalg.norm(a)                                # a random roll about z
        Rm = np.stack([x, np.cross(z, x), z])                    # rows: the camera's axes in the world; q = Rm (X - ctr)
        cams[c, :9] = Rm.T.ravel()                               # column-major
        cams[c, 9:12] = -Rm @ ctr
    cams[:, 12] = rng.uniform(0.8, 1.2, DOME_N_CAM)
    cams[:, 13:15] = rng.uniform(-5e-2, 5e-2, size=(DOME_N_CAM, 2))
    cams[::5, 14] = 0.0
    true_bal9 = O.camera_to_bal(cams)
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    pt_idx = np.concatenate(rows).astype(np.uint64)
    uv = O.project_observations(O.camera_from_bal(true_bal9), pts, row_ptr, pt_idx)
    uv = uv + rng.normal(scale=obs_noise, size=uv.shape)
    bal9 = true_bal9.copy()
    bal9[:, :6] += rng.normal(scale=start_noise, size=(DOME_N_CAM, 6))
    moved = pts + rng.normal(scale=start_noise, size=pts.shape)
    return dict(bal9=bal9, cams15=O.camera_from_bal(bal9), pts=moved, row_ptr=row_ptr, pt_idx=pt_idx, uv=uv,
                lengths=lengths, true_bal9=true_bal9, true_pts=pts, bal=not state)


# ---- general-position cameras and points for the noise and statistics passes (no observations) ----
NOISE_CAM_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 300)          # around a wave of 64 cameras and a workgroup of 256 entities
NOISE_PT_COUNTS = (0, 1, 5, 700)
NOISE_COUNT_PAIRS = tuple((c, p) for c in NOISE_CAM_COUNTS for p in NOISE_PT_COUNTS if c + p)
# statistics: one lane, a batch tail, one wave / workgroup +- 1, four workgroups +- 1, the grid cap (512 workgroups of 256) +- 1, and
# four entities per thread at the cap plus a tail
STATS_TOTALS = (1, 2, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 512 * 256 - 1, 512 * 256, 512 * 256 + 1, 4 * 512 * 256 + 3)
NOISE_VARIANTS = (None, "planar", "far", "offset")
PLANAR_Y = 0.625


def noise_problem(n_cam, n_pts, seed, variant=None, tie_at=4):
    """n_cam cameras in general position and n_pts points: random_problem's rotations, f in [0.8, 1.2], k1 and k2 nonzero
    (every camera's three intrinsics are distinct bit patterns), centres and points in a box of +-30.  Point 0 lies
    next to the coordinate origin -- the drift origin whenever there is a point -- and point tie_at (if there is one) repeats it: a
    tie for the origin search, which the later one wins.  The translation is t = -R c taken in long double and rounded once.
      planar  every centre and every point has y = PLANAR_Y (a zero dimension); only cameras for which the device's
              centre formula returns that y bit for bit are kept (the oracle's center() has the device's order);
      far     a box of +-200: extent 400;
      offset  the cloud moved to (1e6, 1e6, 1e6)-ish with a spread of 1e-3.
    Prefixes of both tables are problems of the same kind.  Returns dict(cams15 [n_cam, 15], pts [n_pts, 3])."""
    assert variant in NOISE_VARIANTS
    rng = np.random.default_rng(seed)
    half = 200.0 if variant == "far" else 30.0
    LDt = np.longdouble

    def place(m):
        x = rng.uniform(-half, half, size=(m, 3))
        if variant == "planar":
            x[:, 1] = PLANAR_Y
        if variant == "offset":
            x = np.array([1.0e6, 1.25e6, 0.75e6]) + x * (1e-3 / half)
        return x
    cams = np.empty((0, 15))
    while len(cams) < n_cam:
        m = 2 * n_cam + 8
        w = rng.uniform(-np.pi, np.pi, size=(m, 3)) * rng.uniform(0.0, 1.0, size=(m, 1))
        R = np.stack([O.from_rodrigues(wi) for wi in w])                       # column-major
        c = place(m)
        Rrow = R.reshape(m, 3, 3).transpose(0, 2, 1).astype(LDt)
        t = (-np.einsum("nij,nj->ni", Rrow, c.astype(LDt))).astype(np.float64)
        sign = np.where(rng.random((m, 2)) < 0.5, -1.0, 1.0)
        intr = np.column_stack([rng.uniform(0.8, 1.2, m), sign * rng.uniform(1e-3, 1e-2, size=(m, 2))])
        new = np.ascontiguousarray(np.column_stack([R, t, intr]))
        if variant == "planar":
            new = new[np.array([O.center(row)[1] == PLANAR_Y for row in new])]
        cams = np.concatenate([cams, new])
    cams = np.ascontiguousarray(cams[:n_cam])
    assert len(np.unique(cams[:, 12:15].view(np.uint64))) == 3 * n_cam and np.all(cams[:, 13:15] != 0.0)
    pts = place(n_pts)
    if n_pts:
        near = np.array([0.01, -0.02, 0.015])
        if variant == "planar":
            near[1] = PLANAR_Y
        if variant == "offset":
            near = pts.min(axis=0) - 1e-4                                      # the entity nearest (0, 0, 0) of a cloud at +1e6
        pts[0] = near
        if 0 < tie_at < n_pts:
            pts[tie_at] = near
    return dict(cams15=cams, pts=np.ascontiguousarray(pts))


def stats_points(n, seed, variant=None):
    """n points of noise_problem's kind (points only: the large statistics totals); the LAST point repeats the first, so that
    the tie for the origin spans the whole table"""
    return noise_problem(0, n, seed, variant, tie_at=n - 1)["pts"]


NOISE_KINDS = ("drift", "drift_normalized", "noise", "sin")
_noise_base = {}


def noise_base(variant=None):
    """the one 300 x 700 problem of each variant the noise tests slice their count pairs from (read-only, cached)"""
    if variant not in _noise_base:
        P = noise_problem(300, 700, seed={None: 11, "planar": 12, "far": 13, "offset": 14}[variant], variant=variant)
        P["cams15"].setflags(write=False)
        P["pts"].setflags(write=False)
        _noise_base[variant] = P
    return _noise_base[variant]


def noise_edge_cases():
    """(label, kind, variant, n_cam, n_pts, parameter overrides): the edge variants of the noise tests"""
    return [("planar/sin", "sin", "planar", 300, 700, {}),
            ("planar-points/sin", "sin", "planar", 0, 700, {}),
            ("far/drift", "drift", "far", 65, 700, dict(angle_strength=0.3, strength=1e-5)),
            ("rotation_std=4/noise", "noise", None, 300, 700, dict(rotation_std=4.0)),
            ("std=0/drift", "drift", None, 65, 5, dict(std=0.0)),
            ("std=0/noise", "noise", None, 65, 5, dict(translation_std=0.0, rotation_std=0.0, point_std=0.0)),
            ("zero-strength/drift", "drift", None, 65, 5, dict(strength=0.0, angle_strength=0.0))]


def noise_cases():
    out = [("%s/%dx%d" % (k, c, p), k, None, c, p, {}) for k in NOISE_KINDS for (c, p) in NOISE_COUNT_PAIRS]
    return out + noise_edge_cases()


def grid_problem():
    """the axis-aligned grid the oracle comparisons of tests/test_gpu_parity.py run on, with its visibility graph"""
    cams, pts = grid_cameras_points(3, cpb=10, ppb=20, L=5.0)
    ci, pi = grid_candidate_pairs(cams, pts, 10.0)
    uv, keep = O.visibility_pairs(cams, pts, ci, pi, 10.0)
    ci, pi, uv = ci[keep == 1], pi[keep == 1], uv[keep == 1]
    row_ptr = np.zeros(len(cams) + 1, dtype=np.int64)
    np.add.at(row_ptr, ci.astype(np.int64) + 1, 1)
    return dict(cams15=cams, pts=pts, row_ptr=np.cumsum(row_ptr).astype(np.uint64), pt_idx=pi.astype(np.uint64), uv=uv)
