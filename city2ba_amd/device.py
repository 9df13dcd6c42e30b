"""Level-0 launchers over torch CUDA(=HIP) tensors.

torch is plumbing here: it owns device memory, the current stream and torch.distributed (RCCL).
Every function forwards raw device pointers + the current stream handle to the C ABI
(include/city2ba_hip.h); nothing is computed by torch ops."""
import ctypes as C

import torch

from . import _lib as L


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _pn(t, n_rows):
    """pointer of an optional [n_rows][4] f64 table (None -> NULL)"""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64 and tuple(t.shape) == (n_rows, 4), "centers"
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, dtype, name):
    assert t.is_cuda and t.is_contiguous() and t.dtype == dtype, name


_live_workspaces = None     # weak references to every workspace made here (tests check their counters after each test)


def workspace(n_obs, device):
    """Scratch of the in-kernel folds for launches of up to n_obs observations, initialised on the current stream
    (c2b_workspace_init: arrival counters zeroed, magic written).  One workspace serves one launch at a time."""
    global _live_workspaces
    import weakref
    nbytes = L.lib().c2b_workspace_bytes(int(n_obs))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)      # torch allocations are 512-B aligned
    with torch.cuda.device(ws.device):
        L.check(L.lib().c2b_workspace_init(_p(ws), _stream()))
    if _live_workspaces is None:
        _live_workspaces = weakref.WeakSet()
    _live_workspaces.add(ws)
    return ws


def workspace_selfcheck(ws):
    """non-zero arrival counters left in ws (0 = clean; -1 = never initialised); synchronises the current stream"""
    n = C.c_int64(-2)
    with torch.cuda.device(ws.device):
        L.check(L.lib().c2b_workspace_selfcheck(_p(ws), _stream(), C.byref(n)))
    return n.value


def live_workspaces():
    return list(_live_workspaces) if _live_workspaces is not None else []


def cameras_from_bal(bal9):
    _chk(bal9, torch.float64, "bal9")
    n = bal9.shape[0]
    cam15 = torch.empty((n, 15), dtype=torch.float64, device=bal9.device)
    L.check(L.lib().c2b_cameras_from_bal(_p(bal9), n, _p(cam15), _stream()))
    return cam15


def cameras_to_bal(cam15):
    _chk(cam15, torch.float64, "cam15")
    n = cam15.shape[0]
    bal9 = torch.empty((n, 9), dtype=torch.float64, device=cam15.device)
    L.check(L.lib().c2b_cameras_to_bal(_p(cam15), n, _p(bal9), _stream()))
    return bal9


def centers_table(n_cam, device):
    """cen4[n_cam][4]: the compact table of camera centres cameras_prepare_* fill next to camblk and the statistics
    read (32 bytes per camera instead of a 128-byte line of the 256-byte record)"""
    return torch.empty((n_cam, 4), dtype=torch.float64, device=device)


class CameraTable:
    """A camblk table for n_cam cameras, OPAQUE on purpose: the table is blocked in groups of 8 cameras (a group's eight
    light lines, then its J_l tails, centres and pad -- include/city2ba_hip.h) and holds whole groups, so its rows are not records:
    slicing, indexing, .to(), .contiguous() or .clone() of a plain [n, 32] view would silently give truncated or scrambled data.
    What exists instead: data_ptr() for the launchers, clone() (whole groups, storage of its own), records() (a COPY of the logical
    [n_cam][32] records, for looking at), flat (the storage: capacity_doubles() doubles, 1-D) and shape == (n_cam, 32) so that
    callers can read the camera count the way they did."""
    __slots__ = ("flat", "n_cam")

    def __init__(self, n_cam, device, flat=None):
        self.n_cam = int(n_cam)
        need = ((self.n_cam + 7) // 8 * 8) * L.CAMBLK_DOUBLES
        if flat is None:
            flat = torch.empty(need, dtype=torch.float64, device=device)
        if not (flat.is_cuda and flat.dtype == torch.float64 and flat.dim() == 1 and flat.is_contiguous() and flat.numel() >= need
                and flat.data_ptr() % 256 == 0):
            raise ValueError("a camera table for %d cameras needs a contiguous, 256-byte aligned 1-D float64 CUDA tensor of >= %d doubles "
                             "(whole groups of 8 cameras)" % (self.n_cam, need))
        self.flat = flat

    shape = property(lambda self: (self.n_cam, L.CAMBLK_DOUBLES))
    device = property(lambda self: self.flat.device)
    dtype = property(lambda self: self.flat.dtype)
    is_cuda = property(lambda self: True)

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.flat.data_ptr()

    def capacity_doubles(self):
        return self.flat.numel()

    def clone(self):
        return CameraTable(self.n_cam, self.flat.device, self.flat.clone())

    def prefix(self, n_cam):
        """the same storage seen as a table of its first n_cam cameras (a camera's place depends on its index only, so a PREFIX
        is a table; any other range is not -- a shard prepares a table of its own)"""
        if not 0 <= int(n_cam) <= self.n_cam:
            raise ValueError("prefix of %d cameras of a table of %d" % (int(n_cam), self.n_cam))
        return CameraTable(n_cam, self.flat.device, self.flat)

    def records(self):
        g = (self.n_cam + 7) // 8
        flat = self.flat[: g * 256].view(g, 256)
        parts = (flat[:, :128].reshape(g, 8, 16), flat[:, 128:192].reshape(g, 8, 8), flat[:, 192:224].reshape(g, 8, 4), flat[:, 224:].reshape(g, 8, 4))
        return torch.cat(parts, dim=-1).reshape(g * 8, L.CAMBLK_DOUBLES)[: self.n_cam].clone()

    def __getitem__(self, _):
        raise TypeError("a CameraTable is not a tensor of records (it is blocked in groups of 8 cameras): use .records() to look at it")

    def __len__(self):
        return self.n_cam


def camblk_table(n_cam, device):
    """an uninitialised camera table for n_cam cameras (CameraTable: storage for whole groups of 8)"""
    return CameraTable(n_cam, device)


def camblk_records(camblk):
    """the table's logical records, [n_cam][CAMBLK_DOUBLES] (R 9, t 3, intrinsics 3, J_l 9, centre 3, pad), as a COPY taken out of
    the blocked layout -- for looking at; the kernels take the table itself"""
    return _as_table(camblk).records()


def camblk_clone(camblk):
    """a copy of a prepared table in storage of its own"""
    return _as_table(camblk).clone()


def _as_table(x, n_cam=None):
    """`out=` arguments and hand-made tables: a CameraTable passes; a tensor is accepted only if its STORAGE from its first
    element on holds whole groups for its row count (what the kernel will write), and is wrapped -- never written out of bounds"""
    if isinstance(x, CameraTable):
        if n_cam is not None and x.n_cam != int(n_cam):
            raise ValueError("the camera table was made for %d cameras, not %d" % (x.n_cam, int(n_cam)))
        return x
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()):
        raise ValueError("camblk: a CameraTable (device.camblk_table) or a contiguous float64 CUDA tensor")
    n = int(n_cam) if n_cam is not None else (x.shape[0] if x.dim() == 2 else x.numel() // L.CAMBLK_DOUBLES)
    need = ((n + 7) // 8 * 8) * L.CAMBLK_DOUBLES
    have = (x.untyped_storage().nbytes() - 8 * x.storage_offset()) // 8
    if have < need:
        raise ValueError("camblk for %d cameras needs %d doubles of storage (whole groups of 8 cameras), this tensor has %d: "
                         "allocate with device.camblk_table()" % (n, need, have))
    return CameraTable(n, x.device, torch.as_strided(x, (need,), (1,)))


def cameras_prepare_state(cam15, out=None, centers=None):
    """the camera table from the in-memory cameras; `centers` (centers_table) also receives every camera's centre"""
    _chk(cam15, torch.float64, "cam15")
    n = cam15.shape[0]
    blk = _as_table(out, n) if out is not None else CameraTable(n, cam15.device)
    L.check(L.lib().c2b_camblk_from_state(_p(cam15), n, _p(blk), blk.capacity_doubles(), _pn(centers, n), _stream()))
    return blk


def cameras_prepare_bal(bal9, out=None, centers=None):
    _chk(bal9, torch.float64, "bal9")
    n = bal9.shape[0]
    blk = _as_table(out, n) if out is not None else CameraTable(n, bal9.device)
    L.check(L.lib().c2b_camblk_from_bal(_p(bal9), n, _p(blk), blk.capacity_doubles(), _pn(centers, n), _stream()))
    return blk


def points_pad(pts3):
    _chk(pts3, torch.float64, "pts3")
    n = pts3.shape[0]
    pts4 = torch.empty((n, 4), dtype=torch.float64, device=pts3.device)
    L.check(L.lib().c2b_points_pad(_p(pts3), n, _p(pts4), _stream()))
    return pts4


def expand_rows(row_ptr, n_obs, obs_base=0):
    _chk(row_ptr, torch.int64, "row_ptr")       # u64 values < 2^63 share the int64 bit pattern
    n_cam = row_ptr.shape[0] - 1
    cam_idx = torch.empty(n_obs, dtype=torch.int32, device=row_ptr.device)
    L.check(L.lib().c2b_expand_rows(_p(row_ptr), n_cam, int(obs_base), int(n_obs), _p(cam_idx), _stream()))
    return cam_idx


def project(camblk, pts4, cam_idx, pt_idx, uv_out):
    L.check(L.lib().c2b_project(_p(camblk), _p(pts4), _p(cam_idx), _p(pt_idx), cam_idx.shape[0], _p(uv_out),
                                _stream()))
    return uv_out


def reprojection_error_sum(camblk, pts4, cam_idx, pt_idx, uv, norm, ws, out_sum):
    L.check(L.lib().c2b_reprojection_error_sum(_p(camblk), _p(pts4), _p(cam_idx), _p(pt_idx), _p(uv),
                                               cam_idx.shape[0], float(norm), _p(ws), _p(out_sum), _stream()))
    return out_sum


class Rows:
    """A camera-major observation list addressed through its row structure -- the reference's one list per camera
    (vis_graph, src/baproblem.rs:256-260) -- instead of a 4-byte camera index per observation: row_ptr [n_cam + 1]
    (int64 tensor holding the u64 values) plus the tile records c2b_rows_pack derives from it (16 bytes per 64
    observations).  The *_rows launchers give the same bits as their cam_idx forms and read ~3.7 bytes per observation
    less."""

    def __init__(self, row_ptr, n_obs=None):
        _chk(row_ptr, torch.int64, "row_ptr")
        self.row_ptr = row_ptr
        self.n_cam = row_ptr.shape[0] - 1
        self.n_obs = int(row_ptr[-1].item()) if n_obs is None else int(n_obs)
        self.tiles = torch.empty((L.lib().c2b_rows_tiles_bytes(self.n_obs) // 16, 4), dtype=torch.int32, device=row_ptr.device)
        L.check(L.lib().c2b_rows_pack(_p(row_ptr), self.n_cam, self.n_obs, _p(self.tiles), _stream()))


def project_rows(camblk, pts4, rows, pt_idx, uv_out):
    L.check(L.lib().c2b_project_rows(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(rows.tiles), _p(pt_idx),
                                     rows.n_obs, _p(uv_out), _stream()))
    return uv_out


def reprojection_error_sum_rows(camblk, pts4, rows, pt_idx, uv, norm, ws, out_sum):
    L.check(L.lib().c2b_reprojection_error_sum_rows(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(rows.tiles),
                                                    _p(pt_idx), _p(uv), rows.n_obs, float(norm), _p(ws), _p(out_sum),
                                                    _stream()))
    return out_sum


def reprojection_error_sums2_rows(camblk, pts4, rows, pt_idx, uv, ws, out_sums):
    """out_sums[0] = the L1 sum, out_sums[1] = the L2 sum, ONE pass (what run_noise evaluates back to back,
    src/bin/city2ba.rs:283-287, 350-354); each bit-identical to reprojection_error_sum_rows with that norm"""
    L.check(L.lib().c2b_reprojection_error_sums2_rows(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(rows.tiles),
                                                      _p(pt_idx), _p(uv), rows.n_obs, _p(ws), _p(out_sums), _stream()))
    return out_sums


def add_noise_observations_error_sums2_rows(camblk, pts4, rows, pt_idx, uv, obs_base, observations_std, seed, ws, out_sums):
    """add_noise's observation pass (src/noise.rs:152-170) fused with the L1 / L2 error sums of the perturbed
    observations (src/bin/city2ba.rs:350-354): uv is perturbed in place exactly as add_noise_observations would"""
    L.check(L.lib().c2b_add_noise_observations_error_sums2_rows(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam,
                                                                _p(rows.tiles), _p(pt_idx), _p(uv), rows.n_obs, int(obs_base),
                                                                float(observations_std), int(seed), _p(ws), _p(out_sums),
                                                                _stream()))
    return out_sums


def visibility_rows(camblk, pts4, rows, pt_idx, max_dist, uv_out, keep):
    L.check(L.lib().c2b_visibility_rows(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(rows.tiles), _p(pt_idx),
                                        rows.n_obs, float(max_dist), _p(uv_out), _p(keep), _stream()))


def visibility_rows_bits(camblk, pts4, rows, pt_idx, max_dist, uv_out, keep_bits):
    """visibility_rows with the mask as one 64-bit word per 64 pairs (keep_bits: int64 tensor of ceil(n / 64) words)"""
    L.check(L.lib().c2b_visibility_rows_bits(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(rows.tiles), _p(pt_idx),
                                             rows.n_obs, float(max_dist), _p(uv_out), _p(keep_bits), _stream()))


def residual_keep_rows(camblk, pts4, rows, pt_idx, uv, max_error, keep, in_front=False):
    """the outlier filter's mask (c2b_residual_keep_rows): keep [n_obs] uint8, 1 where |projected - observed|^2 <=
    max_error^2 (and, with in_front, the point is in front of its camera); a NaN residual gives 0"""
    L.check(L.lib().c2b_residual_keep_rows(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(rows.tiles), _p(pt_idx), _p(uv),
                                           rows.n_obs, float(max_error), L.FILTER_IN_FRONT if in_front else 0, _p(keep), _stream()))
    return keep


def triangulate_rows(camblk, pts4, prows, uv, status, counts, min_angle, pt_mask=None):
    """linear midpoint triangulation (c2b_triangulate_rows): pts4 [n_pts,4] in place from each point's observations
    (PointRows); status [n_pts] uint8 (_lib.TRI_STATUS order), counts [5] int64 = how many points took each status;
    min_angle in radians; pt_mask [n_pts] uint8 (1 = constant) or None"""
    L.check(L.lib().c2b_triangulate_rows(_p(camblk), _p(pts4), prows.n_pts, _p(prows.pt_row_ptr), _p(prows.obs_of), _p(prows.cam_of),
                                         _p(uv), float(min_angle), _p(pt_mask), _p(status), _p(counts), _stream()))
    return status, counts


def refine_points_rows(camblk, pts4, prows, uv, status, counts, rounds=10, lam=1e-4, function_tol=0.0, gradient_tol=0.0, parameter_tol=0.0,
                       loss=None, loss_scale=1.0, prior_pt=None, prior_pt_w=None, pt_mask=None):
    """per-point Levenberg-Marquardt (c2b_refine_points_rows): pts4 [n_pts,4] in place, every point re-minimised
    by itself over its observations (PointRows) with the cameras held; status [n_pts] uint8 (_lib.REFINE_STATUS order),
    counts [6] int64 (_lib.REFINE_COUNTS: the five statuses, then the points written); loss by name with its scale;
    prior_pt / prior_pt_w [n_pts,3] (in pairs) and pt_mask [n_pts] uint8 (1 = constant) or None"""
    import ctypes as C
    opt = L.RefineOptions(int(rounds), 0, float(lam), float(function_tol), float(gradient_tol), float(parameter_tol))
    L.check(L.lib().c2b_refine_points_rows(_p(camblk), _p(pts4), prows.n_pts, _p(prows.pt_row_ptr), _p(prows.obs_of), _p(prows.cam_of),
                                           _p(uv), L.loss_kind(loss), float(loss_scale) * float(loss_scale), _p(prior_pt), _p(prior_pt_w),
                                           C.cast(C.pointer(opt), C.c_void_p), _p(pt_mask), _p(status), _p(counts), _stream()))
    return status, counts


def refine_cameras_rows(bal9, pts4, rows, pt_idx, uv, status, counts, rounds=10, lam=1e-4, function_tol=0.0, gradient_tol=0.0,
                        parameter_tol=0.0, loss=None, loss_scale=1.0, prior_center=None, prior_center_w=None, prior_intr=None,
                        prior_intr_w=None, cam_mask=None):
    """per-camera Levenberg-Marquardt (c2b_refine_cameras_rows): bal9 [n_cam,9] in place, every camera re-minimised
    by itself over its row of observations (Rows) with the points held; status [n_cam] uint8 (_lib.REFINE_STATUS order) or
    None, counts [6] int64 (_lib.REFINE_COUNTS: the five statuses, then the cameras written); loss by name with its scale;
    the centre and intrinsics priors [n_cam,3] (targets and weights, in pairs) and cam_mask [n_cam] uint16 (an OR of
    C2B_CONST_* bits) or None"""
    import ctypes as C
    opt = L.RefineOptions(int(rounds), 0, float(lam), float(function_tol), float(gradient_tol), float(parameter_tol))
    L.check(L.lib().c2b_refine_cameras_rows(_p(bal9), _p(pts4), rows.n_cam, _p(rows.row_ptr), _p(pt_idx), _p(uv), L.loss_kind(loss),
                                            float(loss_scale) * float(loss_scale), _p(prior_center), _p(prior_center_w), _p(prior_intr),
                                            _p(prior_intr_w), C.cast(C.pointer(opt), C.c_void_p), _p(cam_mask), _p(status), _p(counts),
                                            _stream()))
    return status, counts


def triangulate_consensus_rows(camblk, pts4, prows, uv, status, counts, min_angle, max_error, min_inliers=3, max_hypotheses=64,
                               pt_mask=None, hyp=None, n_inl=None, inlier=None):
    """consensus triangulation (c2b_triangulate_consensus_rows): triangulate_rows over the rays of a point that agree with
    each other; status [n_pts] uint8 (_lib.TRI_CONSENSUS_STATUS order), counts [6] int64; hyp, n_inl [n_pts] int32 and
    inlier [n_obs] uint8 (0 = an observation of a triangulated point that is not an inlier) or None; min_angle in radians"""
    L.check(L.lib().c2b_triangulate_consensus_rows(_p(camblk), _p(pts4), prows.n_pts, _p(prows.pt_row_ptr), _p(prows.obs_of),
                                                   _p(prows.cam_of), _p(uv), prows.n_obs, float(min_angle), float(max_error),
                                                   int(min_inliers), int(max_hypotheses), _p(pt_mask), _p(status), _p(hyp), _p(n_inl),
                                                   _p(inlier), _p(counts), _stream()))
    return status, counts


def resect_rows(bal9, pts4, rows, pt_idx, uv, status, counts, min_points=6, min_gap=1e-4, cam_mask=None):
    """camera resection (c2b_resect_rows): bal9 [n_cam,9] in place (entries 0..5; 6..8 are the intrinsics read) from each
    camera's row of observations (Rows); status [n_cam] uint8 (_lib.RES_STATUS order), counts [5] int64 = how many cameras
    took each status; cam_mask [n_cam] uint16 (an OR of C2B_CONST_* bits: a pose bit keeps the camera) or None"""
    L.check(L.lib().c2b_resect_rows(_p(bal9), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(pt_idx), _p(uv), int(min_points), float(min_gap),
                                    _p(cam_mask), _p(status), _p(counts), _stream()))
    return status, counts


def resect_consensus_rows(bal9, pts4, rows, pt_idx, uv, status, counts, max_error, min_inliers=6, min_gap=1e-4, max_hypotheses=64,
                          cam_mask=None, hyp=None, n_inl=None, inlier=None):
    """consensus resection (c2b_resect_consensus_rows): resect_rows over the observations of a camera that agree with each
    other; status [n_cam] uint8 (_lib.RES_CONSENSUS_STATUS order), counts [6] int64; hyp, n_inl [n_cam] int32 and inlier
    [n_obs] uint8 (0 = an observation of a resected camera that is not an inlier) or None"""
    L.check(L.lib().c2b_resect_consensus_rows(_p(bal9), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(pt_idx), _p(uv), rows.n_obs, float(max_error),
                                              int(min_inliers), float(min_gap), int(max_hypotheses), _p(cam_mask), _p(status), _p(hyp), _p(n_inl),
                                              _p(inlier), _p(counts), _stream()))
    return status, counts


def merge_partner_rows(camblk, pts4, prows, uv, partner, status, counts, radius, max_error, pt_held=None):
    """one round's partner choice of landmark merging (c2b_merge_partner_rows): partner [n_pts] int32 = the nearest other
    point within `radius` that shares no camera with the point and whose merged position reprojects every observation of
    both within max_error in front of its camera, or -1; status [n_pts] uint8 (_lib.MERGE_STATUS order), counts [4] int64;
    pt_held [n_pts] uint8 (1 = takes no part) or None.  pts4 is only read.  Synchronises the stream."""
    L.check(L.lib().c2b_merge_partner_rows(_p(camblk), _p(pts4), prows.n_pts, _p(prows.pt_row_ptr), _p(prows.obs_of), _p(prows.cam_of),
                                           _p(uv), prows.n_obs, float(radius), float(max_error), _p(pt_held), _p(partner), _p(status),
                                           _p(counts), _stream()))
    return partner, status, counts


def rematch_rows(camblk, pts4, rows, pt_idx, uv, fits, choice, status, counts, radius, max_error, pt_trusted=None):
    """guided re-matching's choice (c2b_rematch_rows): for every observation that does not fit the point it names -- fits
    [n_obs] uint8, residual_keep_rows(..., in_front=True) at the same max_error -- and whose point is trusted, choice [n_obs]
    int32 = the trusted point it fits best among the neighbours of the named point within `radius` and the labels the
    camera's other failing observations give up, not held by an observation of the camera that stays, or -1; status [n_obs]
    uint8 (_lib.REMATCH_STATUS order) after the conflicts inside each camera are resolved, counts [4] int64; pt_trusted
    [n_pts] uint8 or None (every finite point).  Nothing is applied: pts4, pt_idx and uv are only read.  Synchronises the
    stream."""
    n_pts = pts4.shape[0]
    L.check(L.lib().c2b_rematch_rows(_p(camblk), _p(pts4), n_pts, _p(rows.row_ptr), rows.n_cam, _p(pt_idx), _p(uv), rows.n_obs, _p(fits),
                                     _p(pt_trusted), float(radius), float(max_error), _p(choice), _p(status), _p(counts), _stream()))
    return choice, status, counts


def drop_keep_rows(row_ptr, n_obs, keep_fraction, seed, keep):
    """drop_features' keep bits (c2b_drop_keep_rows): keep [n_obs] uint8 = 1 for the floor(len * keep_fraction)
    observations of every camera row (row_ptr [n_cam + 1] uint64-valued int64) with the smallest (draw, index)"""
    L.check(L.lib().c2b_drop_keep_rows(_p(row_ptr), row_ptr.shape[0] - 1, int(n_obs), float(keep_fraction), int(seed), _p(keep), _stream()))
    return keep


def mismatch_partner_rows(row_ptr, uv, mismatch_chance, seed, partner, n_zero_rows):
    """add_incorrect_correspondences' partner pass (c2b_mismatch_partner_rows): partner [n_obs] int32 = the row-relative index
    the observation swaps its point with, or -1; n_zero_rows [1] int64 = the rows with a swapping observation whose weights are
    all zero.  uv [n_obs, 2] float64."""
    L.check(L.lib().c2b_mismatch_partner_rows(_p(row_ptr), row_ptr.shape[0] - 1, _p(uv), uv.shape[0], float(mismatch_chance), int(seed),
                                              _p(partner), _p(n_zero_rows), _stream()))
    return partner, n_zero_rows


def select_smallest_keys_rows(n, n_select, select, seed=0, stream=0, slot=0, keys=None):
    """select [n] uint8 = 1 for the n_select smallest (key, index) (c2b_select_smallest_keys_rows): keys [n] int64 holding
    uint64 bit patterns, or None for the draws a of (seed; stream, entity = index, slot).  Synchronises the stream."""
    L.check(L.lib().c2b_select_smallest_keys_rows(_p(keys), int(n), int(seed), int(stream), int(slot), int(n_select), _p(select), _stream()))
    return select


def nearest_points_rows(pts4, query, nearest):
    """nearest [n_query, 11] int32 = the nearest points of the points query [n_query] (int32-valued uint32) of pts4 [n_pts, 4]
    by ascending (d2, index), the point itself included; -1 past the table's size (c2b_nearest_points_rows).  Synchronises."""
    L.check(L.lib().c2b_nearest_points_rows(_p(pts4), pts4.shape[0], _p(query), query.shape[0], _p(nearest), _stream()))
    return nearest


def residual_jacobian_rows(camblk, pts4, rows, pt_idx, uv, r, Jc, Jp, norm=2.0, ws=None, out_sum=None, obs_base=0,
                           n_obs=None):
    """residual + Jacobian (+ sum |r|^norm when ws is given: into out_sum, or into ws for error_sum_finish) of the
    observations [obs_base, obs_base + n_obs) of the list `rows` describes; pt_idx / uv / r / Jc / Jp are that slice."""
    n = rows.n_obs - int(obs_base) if n_obs is None else int(n_obs)
    tiles = rows.tiles[int(obs_base) // 64:]
    L.check(L.lib().c2b_residual_jacobian_rows(_p(camblk), _p(pts4), pts4.shape[0], _p(rows.row_ptr), rows.n_cam, _p(tiles),
                                               int(obs_base), _p(pt_idx), _p(uv), n, _p(r), _p(Jc), _p(Jp),
                                               float(norm), _p(ws), _p(out_sum), _stream()))
    return out_sum


def jacobian_stream_policy(n_obs, n_cam, n_pts):
    """0 / 2 / 3: which once-read streams of a residual_jacobian_rows launch of this size bypass the caches"""
    return int(L.lib().c2b_jacobian_stream_policy(int(n_obs), int(n_cam), int(n_pts)))


def jacobian_tiles_per_wave(n_obs):
    return int(L.lib().c2b_jacobian_tiles_per_wave(int(n_obs)))


def jacobian_launch_shape(n_obs, store_GBs=0.0):
    """(waves per workgroup, tiles of 64 observations per wave) of a residual_jacobian_rows launch of this size into an
    output set that takes streaming stores at store_GBs (0 = unknown)"""
    w, t = C.c_int(0), C.c_int(0)
    L.check(L.lib().c2b_jacobian_launch_shape(int(n_obs), float(store_GBs), C.byref(w), C.byref(t)))
    return w.value, t.value


def residual_jacobian_rows_placed(camblk, pts4, rows, pt_idx, uv, outputs, norm=2.0, ws=None, out_sum=None):
    """residual_jacobian_rows over the whole list into a placed output set (JacobianOutputs): the launch takes the
    workgroup shape that suits the store rate measured for that set"""
    L.check(L.lib().c2b_residual_jacobian_rows_placed(_p(camblk), _p(pts4), pts4.shape[0], _p(rows.row_ptr), rows.n_cam, _p(rows.tiles),
                                                      _p(pt_idx), _p(uv), rows.n_obs, outputs.handle, float(norm), _p(ws), _p(out_sum),
                                                      _stream()))
    return out_sum


class PointRows:
    """The point-major transpose of a camera-major list (c2b_normal_transpose): pt_row_ptr [n_pts + 1] (int64 holding
    u64), obs_of [n_obs] -- each point's observations in ascending order, a stable argsort of pt_idx -- and cam_of [n_obs],
    the camera of obs_of[j] (int32 tensors holding u32).  What normal_points_rows walks."""

    def __init__(self, rows, pt_idx, n_pts):
        _chk(pt_idx, torch.int32, "pt_idx")
        dev = rows.row_ptr.device
        self.n_pts, self.n_obs = int(n_pts), rows.n_obs
        self.pt_row_ptr = torch.empty(self.n_pts + 1, dtype=torch.int64, device=dev)
        self.obs_of = torch.empty(max(self.n_obs, 1), dtype=torch.int32, device=dev)[:self.n_obs]
        self.cam_of = torch.empty(max(self.n_obs, 1), dtype=torch.int32, device=dev)[:self.n_obs]
        temp = torch.empty((L.lib().c2b_normal_transpose_temp_bytes(self.n_obs, self.n_pts) + 7) // 8, dtype=torch.float64, device=dev)
        L.check(L.lib().c2b_normal_transpose(_p(rows.row_ptr), rows.n_cam, _p(pt_idx), self.n_obs, self.n_pts, _p(self.pt_row_ptr),
                                             _p(self.obs_of), _p(self.cam_of), _p(temp), _stream()))
        temp.record_stream(torch.cuda.current_stream(dev))


COVIS_WAVE_SLOTS = 2048     # C2B_COVIS_WAVE_SLOTS: slots of the LDS table a wave counts one camera's neighbours in


def _covis_temp(n_cam, which, device):
    return torch.empty((L.lib().c2b_covisibility_temp_bytes(int(n_cam), which) + 7) // 8, dtype=torch.float64, device=device)


def covisibility_rows(rows, pt_idx, prows, min_shared=1, return_counts=False):
    """the camera covisibility graph of a camera-major list (c2b_covisibility_degree_rows / _fill_rows): rows (Rows),
    pt_idx [n_obs] int32, prows (PointRows of the same list).  Returns (nbr_ptr [n_cam + 1] int64 holding u64, nbr [n_edges],
    shared [n_edges] int32 holding u32): per camera its neighbours in ascending index -- the cameras that observe at least
    min_shared distinct points it observes too -- and the number shared.  With return_counts also the int64 [2] tensor
    (n_edges, cameras that took the heavy path).  Synchronises the stream once, to size the outputs."""
    dev = rows.row_ptr.device
    n_cam = rows.n_cam
    temp = _covis_temp(n_cam, L.COVIS_TEMP_GRAPH, dev)
    nbr_ptr = torch.empty(n_cam + 1, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    args = (_p(rows.row_ptr), _p(pt_idx), _p(prows.pt_row_ptr), _p(prows.obs_of), _p(prows.cam_of), n_cam, prows.n_pts, rows.n_obs, int(min_shared), _p(temp))
    L.check(L.lib().c2b_covisibility_degree_rows(*args, _p(nbr_ptr), _p(counts), _stream()))
    n_edges = int(counts[0].item())
    nbr = torch.empty(max(n_edges, 1), dtype=torch.int32, device=dev)             # (never a NULL pointer)
    shared = torch.empty(max(n_edges, 1), dtype=torch.int32, device=dev)
    L.check(L.lib().c2b_covisibility_fill_rows(*args, _p(nbr_ptr), _p(nbr), _p(shared), _stream()))
    temp.record_stream(torch.cuda.current_stream(dev))
    nbr, shared = nbr[:n_edges], shared[:n_edges]
    return (nbr_ptr, nbr, shared, counts) if return_counts else (nbr_ptr, nbr, shared)


def covisibility_expand_rows(nbr_ptr, nbr, shared, frontier, hop, level, min_shared=1, within=None):
    """one level of a breadth-first search over a covisibility graph (c2b_covisibility_expand_rows): level [n_cam] int32 in place
    (-1 = not reached), frontier [n] int32 = the cameras of level `hop`; their neighbours that are not reached, share at least
    min_shared points and lie inside within [n_cam] uint8 (or None) get level hop + 1.  Returns (next [n_cam] int32, n_next [1]
    int32): the cameras of level hop + 1 in ascending index and their number."""
    dev = level.device
    n_cam = level.shape[0]
    temp = _covis_temp(n_cam, L.COVIS_TEMP_EXPAND, dev)
    nxt = torch.empty(max(n_cam, 1), dtype=torch.int32, device=dev)
    n_next = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(L.lib().c2b_covisibility_expand_rows(_p(nbr_ptr), _p(nbr), _p(shared), n_cam, int(min_shared), _p(within), _p(frontier), frontier.shape[0],
                                                 int(hop), _p(level), _p(nxt), _p(n_next), _p(temp), _stream()))
    temp.record_stream(torch.cuda.current_stream(dev))
    return nxt[:n_cam], n_next


def _loss_args(loss):
    """loss= of the *_rows passes: None, or (name, scale) -- the (kind, scale) of the *_rows_loss entries"""
    if isinstance(loss, str) or not hasattr(loss, "__len__") or len(loss) != 2:
        raise ValueError("loss must be None or (name, scale), e.g. ('cauchy', 0.01), not %r" % (loss,))
    return L.loss_kind(loss[0]), float(loss[1])


def normal_cameras_rows(camblk, pts4, rows, pt_idx, uv, U, gc, ws=None, sum_sq=None, loss=None):
    """camera pass of the Gauss-Newton blocks: U [n_cam,9,9] = sum Jc^T Jc, gc [n_cam,9] = sum Jc^T r over each camera's
    observations (+ sum |r|^2 into sum_sq[0] when ws and sum_sq are given), the Jacobian never stored.  loss = (name,
    scale): every observation reweighted by the robust loss's sqrt(w) first (c2b_normal_cameras_rows_loss)"""
    if loss is not None:
        L.check(L.lib().c2b_normal_cameras_rows_loss(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(pt_idx), _p(uv), rows.n_obs,
                                                     _p(U), _p(gc), _p(ws), _p(sum_sq), *_loss_args(loss), _stream()))
        return U, gc
    L.check(L.lib().c2b_normal_cameras_rows(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(pt_idx), _p(uv), rows.n_obs,
                                            _p(U), _p(gc), _p(ws), _p(sum_sq), _stream()))
    return U, gc


def normal_points_rows(camblk, pts4, prows, uv, V, gp, loss=None):
    """point pass: V [n_pts,3,3] = sum Jp^T Jp, gp [n_pts,3] = sum Jp^T r over each point's observations (PointRows);
    loss = (name, scale) as in normal_cameras_rows"""
    if loss is not None:
        L.check(L.lib().c2b_normal_points_rows_loss(_p(camblk), _p(pts4), prows.n_pts, _p(prows.pt_row_ptr), _p(prows.obs_of),
                                                    _p(prows.cam_of), _p(uv), _p(V), _p(gp), *_loss_args(loss), _stream()))
        return V, gp
    L.check(L.lib().c2b_normal_points_rows(_p(camblk), _p(pts4), prows.n_pts, _p(prows.pt_row_ptr), _p(prows.obs_of), _p(prows.cam_of),
                                           _p(uv), _p(V), _p(gp), _stream()))
    return V, gp


def schur_points_rows(camblk, pts4, prows, uv, V, lam, x, h, t, loss=None):
    """point pass of the damped step's Schur complement: t [n_pts,3] = V_l^-1 (h + sum Jp^T (Jc x)) per point (PointRows),
    V_l = V damped by lam (c2b_schur_points_rows); x [n_cam,9] None means 0, h [n_pts,3] None means 0; loss = (name,
    scale): Jc, Jp of the reweighted system (V must be its V)"""
    if loss is not None:
        L.check(L.lib().c2b_schur_points_rows_loss(_p(camblk), _p(pts4), prows.n_pts, _p(prows.pt_row_ptr), _p(prows.obs_of),
                                                   _p(prows.cam_of), _p(uv), _p(V), float(lam), _p(x), _p(h), _p(t), *_loss_args(loss),
                                                   _stream()))
        return t
    L.check(L.lib().c2b_schur_points_rows(_p(camblk), _p(pts4), prows.n_pts, _p(prows.pt_row_ptr), _p(prows.obs_of), _p(prows.cam_of),
                                          _p(uv), _p(V), float(lam), _p(x), _p(h), _p(t), _stream()))
    return t


def schur_jacobi_blocks(camblk, pts4, rows, pt_idx, uv, U, V, lam, M, loss=None):
    """the Schur-Jacobi preconditioner's blocks: M [n_cam,9,9] = lam diag(d_c) + sum Jc^T (I - Jp V_l^-1 Jp^T) Jc per camera,
    d_c the damping diagonal of U's block (c2b_schur_jacobi_rows) -- the diagonal blocks of the Schur complement when no
    camera sees a point twice.  U, V as normal_cameras_rows / normal_points_rows filled them; loss as there"""
    if loss is not None:
        L.check(L.lib().c2b_schur_jacobi_rows_loss(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(pt_idx), _p(uv), rows.n_obs,
                                                   _p(U), _p(V), float(lam), _p(M), *_loss_args(loss), _stream()))
        return M
    L.check(L.lib().c2b_schur_jacobi_rows(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(pt_idx), _p(uv), rows.n_obs,
                                          _p(U), _p(V), float(lam), _p(M), _stream()))
    return M


def schur_cameras_rows(camblk, pts4, rows, pt_idx, uv, U, lam, x, t, y, loss=None):
    """camera pass: y [n_cam,9] = U_l x - sum Jc^T (Jp t) per camera, U_l = U damped by lam (c2b_schur_cameras_rows);
    x None drops the U term.  S x = schur_cameras_rows(.., x, schur_points_rows(.., x, None, t), y); loss as there"""
    if loss is not None:
        L.check(L.lib().c2b_schur_cameras_rows_loss(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(pt_idx), _p(uv), rows.n_obs,
                                                    _p(U), float(lam), _p(x), _p(t), _p(y), *_loss_args(loss), _stream()))
        return y
    L.check(L.lib().c2b_schur_cameras_rows(_p(camblk), _p(pts4), _p(rows.row_ptr), rows.n_cam, _p(pt_idx), _p(uv), rows.n_obs,
                                           _p(U), float(lam), _p(x), _p(t), _p(y), _stream()))
    return y


SCHUR_LDS_BLOCKS = 32       # C2B_SCHUR_LDS_BLOCKS: a row of at most this many neighbours accumulates its blocks of S in LDS


def schur_y_rows(camblk, pts4, cam_idx, pt_idx, uv, V, lam, Y, loss=None):
    """per observation Y [n_obs,3,9] = L^-1 Jp^T Jc with V_l = L L^T of the observation's point (c2b_schur_y_rows):
    cam_idx [n_obs] int32 (expand_rows), V as normal_points_rows filled it; W_o V_l^-1 W_o'^T = Y_o^T Y_o' for two
    observations of one point.  loss as in normal_cameras_rows"""
    n_obs = pt_idx.shape[0]
    if loss is not None:
        L.check(L.lib().c2b_schur_y_rows_loss(_p(camblk), _p(pts4), _p(cam_idx), _p(pt_idx), _p(uv), n_obs, _p(V), float(lam), _p(Y),
                                              *_loss_args(loss), _stream()))
        return Y
    L.check(L.lib().c2b_schur_y_rows(_p(camblk), _p(pts4), _p(cam_idx), _p(pt_idx), _p(uv), n_obs, _p(V), float(lam), _p(Y), _stream()))
    return Y


def schur_blocks_rows(rows, pt_idx, prows, nbr_ptr, nbr, Y, S_diag, S_off):
    """the blocks of the explicit Schur complement on the pattern (nbr_ptr, nbr) = covisibility_rows(rows, pt_idx, prows, 1)
    (c2b_schur_blocks_rows): S_off [n_edges,9,9] written, both (c, c') and its transpose at (c', c); the cross terms of
    duplicated (camera, point) pairs added to S_diag [n_cam,9,9], which holds schur_jacobi_blocks' M on entry and S's
    diagonal blocks on exit"""
    L.check(L.lib().c2b_schur_blocks_rows(_p(rows.row_ptr), _p(pt_idx), _p(prows.pt_row_ptr), _p(prows.obs_of), _p(prows.cam_of), rows.n_cam,
                                          rows.n_obs, _p(nbr_ptr), _p(nbr), _p(Y), _p(S_diag), _p(S_off), _stream()))
    return S_diag, S_off


def schur_spmv_rows(nbr_ptr, nbr, S_diag, S_off, x, y, part=None):
    """y [n_cam,9] = S x with the stored blocks (c2b_schur_spmv_rows); part [4 ceil(n_cam / 4)], when given, takes x.y as one
    partial per wave"""
    L.check(L.lib().c2b_schur_spmv_rows(_p(nbr_ptr), _p(nbr), S_diag.shape[0], _p(S_diag), _p(S_off), _p(x), _p(y), _p(part), _stream()))
    return y


DENSE_MAX_CAMERAS = 4096    # C2B_DENSE_MAX_CAMERAS: the dense image's leading dimension is at most 9 times this


def dense_scatter_rows(nbr_ptr, nbr, S_diag, S_off, A):
    """the lower triangle of S = (S_diag [n_cam,9,9], S_off [n_edges,9,9] on the pattern nbr_ptr, nbr) into the dense image
    A [Np, ld] (c2b_dense_scatter_rows), Np = 64 ceil(9 n_cam / 64) <= ld = A.shape[1], ld a multiple of 64: zeros
    elsewhere in the lower triangle, the padding rows i >= 9 n_cam rows of the identity; the upper triangle is not written"""
    L.check(L.lib().c2b_dense_scatter_rows(_p(nbr_ptr), _p(nbr), S_diag.shape[0], _p(S_diag), _p(S_off), _p(A), A.shape[1], _stream()))
    return A


def dense_cholesky(A, n, info):
    """A [Np, ld] = L L^T in place on the lower triangle (c2b_dense_cholesky): n rows are the matrix, the rows up to
    Np = 64 ceil(n / 64) padding rows of the identity; info [1] int32 takes 0, or the 1-based index of the first pivot that was
    not finite or not > 0 (the factor is then meaningless)"""
    L.check(L.lib().c2b_dense_cholesky(_p(A), int(n), A.shape[1], _p(info), _stream()))
    return A


def dense_cholesky_solve(A, n, x):
    """x [Np] <- L^-T L^-1 x with the factor dense_cholesky left in A (c2b_dense_cholesky_solve); x's padding entries must be finite"""
    L.check(L.lib().c2b_dense_cholesky_solve(_p(A), int(n), A.shape[1], _p(x), _stream()))
    return x


def _prior_pair(target, w, n, name):
    """a (target, weights) pair of a prior: both None, or both [n, 3] float64 on the device"""
    if (target is None) != (w is None):
        raise ValueError("%s: a prior's target and its weights go in pairs" % name)
    for a in (target, w):
        if a is not None:
            _chk(a, torch.float64, name)
            if tuple(a.shape) != (n, 3):
                raise ValueError("%s must have shape (%d, 3)" % (name, n))
    return _p(target), _p(w)


def prior_cameras_rows(camblk, center=None, center_w=None, intr=None, intr_w=None, U=None, gc=None, r=None, A=None, part=None, cost=None):
    """the camera priors' terms (c2b_prior_cameras_rows): U [n_cam,9,9] += A^T A, gc [n_cam,9] += A^T r for r_C = w_C o (C - C0)
    (C the centre of the camera's record) and r_I = w_I o ((f, k1, k2) - I0); any of U, gc None skips it.  r [n_cam,6] and
    A [n_cam,3,6] = diag(w_C) [dC/dw | -R^T] are written when given; part [ceil(9 n_cam / 256)] takes the cost's partials and
    cost [1] their sum.  (center, center_w) and (intr, intr_w) are [n_cam,3] pairs, None together."""
    n = _as_table(camblk).n_cam
    c0, cw = _prior_pair(center, center_w, n, "center")
    i0, iw = _prior_pair(intr, intr_w, n, "intr")
    if part is not None and part.numel() < (9 * n + 255) // 256:
        raise ValueError("prior_cameras_rows: part needs %d doubles" % ((9 * n + 255) // 256))
    L.check(L.lib().c2b_prior_cameras_rows(_p(camblk), n, c0, cw, i0, iw, _p(U), _p(gc), _p(r), _p(A), _p(part), _p(cost), _stream()))
    return U, gc


def prior_points_rows(pts4, pt=None, pt_w=None, V=None, gp=None, r=None, part=None, cost=None):
    """the point priors' terms (c2b_prior_points_rows): V [n_pts,3,3] += diag(w_X^2), gp [n_pts,3] += w_X o r_X, r_X = w_X o
    (X - X0); r [n_pts,3], part [ceil(n_pts / 256)] and cost [1] as in prior_cameras_rows"""
    n = pts4.shape[0]
    x0, xw = _prior_pair(pt, pt_w, n, "pt")
    if part is not None and part.numel() < (n + 255) // 256:
        raise ValueError("prior_points_rows: part needs %d doubles" % ((n + 255) // 256))
    L.check(L.lib().c2b_prior_points_rows(_p(pts4), n, x0, xw, _p(V), _p(gp), _p(r), _p(part), _p(cost), _stream()))
    return V, gp


def prior_model_rows(camblk, pts4, dc, dp, sums, center=None, center_w=None, intr=None, intr_w=None, pt=None, pt_w=None):
    """the priors' part of a step's two sums (c2b_prior_model_rows): sums[0] = sum |r_prior|^2, sums[1] = sum (|r_prior|^2 -
    |r_prior + A delta|^2) for the step dc [n_cam,9], dp [n_pts,3]; sums is a float64 device tensor of 2"""
    nc, npt = _as_table(camblk).n_cam, pts4.shape[0]
    c0, cw = _prior_pair(center, center_w, nc, "center")
    i0, iw = _prior_pair(intr, intr_w, nc, "intr")
    x0, xw = _prior_pair(pt, pt_w, npt, "pt")
    part = torch.empty((2, (max(nc, npt) + 255) // 256 + 1), dtype=torch.float64, device=sums.device)
    L.check(L.lib().c2b_prior_model_rows(_p(camblk), nc, c0, cw, i0, iw, _p(pts4), npt, x0, xw, _p(dc), _p(dp), _p(part[0]), _p(part[1]),
                                         _p(sums), _stream()))
    return sums


def residual_jacobian(camblk, pts4, cam_idx, pt_idx, uv, r, Jc, Jp, norm=2.0, ws=None):
    """ws != None -> the same launch also folds sum |r|^norm into ws (see error_sum_finish)."""
    L.check(L.lib().c2b_residual_jacobian(_p(camblk), _p(pts4), _p(cam_idx), _p(pt_idx), _p(uv), cam_idx.shape[0],
                                          _p(r), _p(Jc), _p(Jp), float(norm), _p(ws), _stream()))


def residual_jacobian_sum(camblk, pts4, cam_idx, pt_idx, uv, r, Jc, Jp, norm, ws, out_sum):
    """residual + Jacobian + sum |r|^norm -> out_sum[0], ONE launch."""
    L.check(L.lib().c2b_residual_jacobian_sum(_p(camblk), _p(pts4), _p(cam_idx), _p(pt_idx), _p(uv), cam_idx.shape[0],
                                              _p(r), _p(Jc), _p(Jp), float(norm), _p(ws), _p(out_sum), _stream()))
    return out_sum


def calib_store_pattern(r, Jc, Jp):
    """Calibration: the residual+Jacobian kernel's store geometry alone (fills r, Jc, Jp with a pattern)."""
    L.check(L.lib().c2b_calib_store_pattern(r.shape[0], _p(r), _p(Jc), _p(Jp), _stream()))


def calib_copy(src, dst):
    """Calibration: 16-bytes-per-lane streaming copy of src into dst (same byte size, multiple of 16)."""
    nbytes = src.numel() * src.element_size()
    assert nbytes == dst.numel() * dst.element_size()
    L.check(L.lib().c2b_calib_copy(_p(src), _p(dst), nbytes, _stream()))


class _DeviceArray:
    """memory owned by a C-ABI handle, exposed to torch through __cuda_array_interface__ (zero copy; the tensor made
    from it keeps this object, and through it the handle, alive)"""

    def __init__(self, ptr, shape, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (int(ptr), False), "version": 2,
                                         "strides": None}
        self._owner = owner


class _OutputsHandle:
    """owns one c2b_jacobian_outputs; freed when the last tensor viewing it (and the JacobianOutputs) is gone.  Kept
    apart from JacobianOutputs so that tensor -> array -> handle holds no reference cycle through torch."""

    def __init__(self):
        self.h = C.c_void_p()

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h and L is not None:                              # (at interpreter shutdown the module globals may be gone already)
            L.lib().c2b_jacobian_outputs_free(h)


class JacobianOutputs:
    """c2b_jacobian_outputs: r [n,2], Jc [n,18], Jp [n,6] in device allocations chosen for streaming-store speed
    (include/city2ba_hip.h).  .r / .Jc / .Jp are torch views of the handle's memory; .log = store
    GB/s of every attempt, .chosen = the attempt kept."""

    def __init__(self, n_obs, device, max_attempts=8, fast_store_GBs=7000.0, _handle=None):
        own = self._own = _OutputsHandle()
        dev = torch.device(device)
        if _handle is not None:                                  # a set the library allocated (c2b_problem_residual_jacobian_device)
            own.h = _handle
        else:
            with torch.cuda.device(dev):
                L.check(L.lib().c2b_jacobian_outputs_alloc(int(n_obs), int(max_attempts), float(fast_store_GBs), _stream(),
                                                           C.byref(own.h)))
        r, jc, jp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(L.lib().c2b_jacobian_outputs_pointers(own.h, C.byref(r), C.byref(jc), C.byref(jp)))
        rates = (C.c_double * 64)()
        na, ch = C.c_int(0), C.c_int(-1)
        L.check(L.lib().c2b_jacobian_outputs_log(own.h, rates, 64, C.byref(na), C.byref(ch)))
        self.log = [round(rates[i], 1) for i in range(na.value)] if n_obs >= 1_000_000 else []
        self.chosen = ch.value
        sr = C.c_double(0.0)
        L.check(L.lib().c2b_jacobian_outputs_store_rate(own.h, C.byref(sr)))
        self.store_GBs = sr.value                                # of the kept set (0: not measured)
        n = max(int(n_obs), 0)
        if n == 0:
            self.r, self.Jc, self.Jp = (torch.empty((0, k), dtype=torch.float64, device=dev) for k in (2, 18, 6))
        else:
            self.r = torch.as_tensor(_DeviceArray(r.value, (n, 2), own), device=dev)
            self.Jc = torch.as_tensor(_DeviceArray(jc.value, (n, 18), own), device=dev)
            self.Jp = torch.as_tensor(_DeviceArray(jp.value, (n, 6), own), device=dev)

    @property
    def handle(self):
        return self._own.h

    def set_store_rate(self, store_GBs):
        """replace the rate the library measured (residual_jacobian_rows_placed chooses its launch shape by it)"""
        L.check(L.lib().c2b_jacobian_outputs_set_store_rate(self._own.h, float(store_GBs)))
        self.store_GBs = max(float(store_GBs), 0.0)


def alloc_jacobian_outputs(n_obs, device, max_attempts=8, fast_store_GBs=7000.0):
    """((r, Jc, Jp), log): the output arrays of residual_jacobian*, placed for streaming stores by the library
    (c2b_jacobian_outputs_alloc -- every caller of the C ABI gets the same placement, not just this wrapper)."""
    out = JacobianOutputs(n_obs, device, max_attempts, fast_store_GBs)
    return (out.r, out.Jc, out.Jp), out.log


def error_sum_finish(ws, n_obs, out_sum):
    L.check(L.lib().c2b_error_sum_finish(_p(ws), int(n_obs), _p(out_sum), _stream()))
    return out_sum


def cameras_from_position_direction(pos3, dir9):
    _chk(pos3, torch.float64, "pos3")
    _chk(dir9, torch.float64, "dir9")
    n = pos3.shape[0]
    cam15 = torch.empty((n, 15), dtype=torch.float64, device=pos3.device)
    L.check(L.lib().c2b_cameras_from_position_direction(_p(pos3), _p(dir9), n, _p(cam15), _stream()))
    return cam15


def visibility_pairs(camblk, pts4, cam_idx, pt_idx, max_dist, uv_out, keep):
    L.check(L.lib().c2b_visibility_pairs(_p(camblk), _p(pts4), _p(cam_idx), _p(pt_idx), cam_idx.shape[0],
                                         float(max_dist), _p(uv_out), _p(keep), _stream()))


def occlusion_filter(camblk, pts4, cam_idx, pt_idx, tri9, keep):
    """occlusion rays of visibility_graph (src/generate.rs:455-476) against f32 triangles [n,9], brute force"""
    _chk(tri9, torch.float32, "tri9")
    L.check(L.lib().c2b_occlusion_filter(_p(camblk), _p(pts4), _p(cam_idx), _p(pt_idx), cam_idx.shape[0], _p(tri9),
                                         tri9.shape[0], _p(keep), _stream()))


class OcclusionBVH:
    """host-built hierarchy over f32 triangles [n,9] placed in device memory; filter() = occlusion_filter through it"""

    def __init__(self, tri9, device):
        import numpy as np
        tri = np.ascontiguousarray(tri9, dtype=np.float32).reshape(-1, 9)
        h = C.c_void_p()
        L.check(L.lib().c2b_bvh_build(tri.ctypes.data_as(C.c_void_p), len(tri), C.byref(h)))
        try:
            nn, ns, depth = C.c_int64(), C.c_int64(), C.c_int()
            L.check(L.lib().c2b_bvh_sizes(h, C.byref(nn), C.byref(ns), C.byref(depth)))
            self.n_nodes, self.n_slots, self.depth = nn.value, ns.value, depth.value
            nodes = np.empty((self.n_nodes, 16), dtype=np.float32)
            tris = np.empty((max(self.n_slots, 1), 12), dtype=np.float32)
            self.order = np.empty(self.n_slots, dtype=np.uint32)
            L.check(L.lib().c2b_bvh_copy(h, nodes.ctypes.data_as(C.c_void_p), tris.ctypes.data_as(C.c_void_p),
                                         self.order.ctypes.data_as(C.c_void_p)))
        finally:
            L.lib().c2b_bvh_free(h)
        self.nodes_host = nodes
        self.nodes = torch.from_numpy(nodes).to(device)
        self.tris = torch.from_numpy(tris).to(device)

    def filter(self, camblk, pts4, cam_idx, pt_idx, keep):
        """keep[i] = 1 iff observation i's ray reaches its point unoccluded.  Raises if a traversal overflowed its
        stack (only possible for node arrays not made by c2b_bvh_build): the mask would be wrong."""
        overflow = torch.zeros(1, dtype=torch.int32, device=keep.device)
        L.check(L.lib().c2b_occlusion_filter_bvh(_p(camblk), _p(pts4), _p(cam_idx), _p(pt_idx), cam_idx.shape[0],
                                                 _p(self.nodes), self.n_nodes, _p(self.tris), self.n_slots, _p(keep),
                                                 _p(overflow), _stream()))
        if int(overflow.item()):
            raise L.City2baError(L.ERR_INVALID_ARGUMENT, "occlusion_filter_bvh: hierarchy deeper than the traversal stack")


def stats(camblk, pts4, ws, out=None, centers=None):
    """centers = the table cameras_prepare_* filled for these cameras (None: the centres are read out of camblk, one
    128-byte line per camera)"""
    out = out if out is not None else torch.empty(L.STATS_DOUBLES, dtype=torch.float64, device=camblk.device)
    L.check(L.lib().c2b_stats(_p(camblk), _pn(centers, camblk.shape[0]), camblk.shape[0], _p(pts4), pts4.shape[0], _p(ws),
                              _p(out), _stream()))
    return out


# ---- similarity alignment, Level 0: x = the estimate's tables, y = the reference's, 32-byte rows [n, 4] ----
def _align_tables(x, y, use, kind):
    if x is None:
        return None, None, None, 0
    for t in (x, y):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == 4 and t.shape == x.shape, kind
    if use is not None:
        assert use.is_cuda and use.is_contiguous() and use.dtype == torch.uint8 and use.shape[0] == x.shape[0], kind + " mask"
    return _p(x), _p(y), _p(use), x.shape[0]


def align_means_rows(ws, x_cam=None, y_cam=None, use_cam=None, x_pts=None, y_pts=None, use_pt=None, out=None):
    """c2b_align_means_rows: out [7] = count, sum x, sum y over the on-correspondences of the pooled tables (a kind may be None)"""
    xc, yc, uc, nc = _align_tables(x_cam, y_cam, use_cam, "cameras")
    xp, yp, up, np_ = _align_tables(x_pts, y_pts, use_pt, "points")
    out = out if out is not None else torch.empty(7, dtype=torch.float64, device=ws.device)
    L.check(L.lib().c2b_align_means_rows(xc, yc, uc, nc, xp, yp, up, np_, _p(ws), _p(out), _stream()))
    return out


def align_moments_rows(ws, means, x_cam=None, y_cam=None, use_cam=None, x_pts=None, y_pts=None, use_pt=None, out=None):
    """c2b_align_moments_rows: out [23] = the eleven moments about the pivot means[1:] / means[0], the six residual sums, the pivot
    (L.align_finish_moments moves them onto the mean)"""
    xc, yc, uc, nc = _align_tables(x_cam, y_cam, use_cam, "cameras")
    xp, yp, up, np_ = _align_tables(x_pts, y_pts, use_pt, "points")
    out = out if out is not None else torch.empty(23, dtype=torch.float64, device=ws.device)
    L.check(L.lib().c2b_align_moments_rows(xc, yc, uc, nc, xp, yp, up, np_, _p(means), _p(ws), _p(out), _stream()))
    return out


def align_errors_rows(ws, x, y, sim, base=None, use=None, max_dist=0.0, err=None, next_=None, out=None):
    """c2b_align_errors_rows: err [n] = |s R x + t - y| (may be None), next_ [n] = base && err <= max_dist (may be None),
    out [7] = count, sum e^2, sum e, max, argmax over `use`, bytes of next_ that differ from use, size of next_.  sim = L.similarity(...)"""
    px, py, _, n = _align_tables(x, y, None, "tables")
    out = out if out is not None else torch.empty(7, dtype=torch.float64, device=ws.device)
    L.check(L.lib().c2b_align_errors_rows(px, py, n, C.byref(sim), _p(base), _p(use), float(max_dist), _p(err), _p(next_), _p(ws), _p(out), _stream()))
    return out


def align_rotation_errors_rows(ws, x_cam15, y_cam15, sim, use=None, err=None, out=None):
    """c2b_align_rotation_errors_rows: err [n] = the angle between R_c R^T and the reference's R_c, out [7] as align_errors_rows"""
    _chk(x_cam15, torch.float64, "x_cam15")
    _chk(y_cam15, torch.float64, "y_cam15")
    assert x_cam15.shape == y_cam15.shape and x_cam15.shape[1] == 15
    out = out if out is not None else torch.empty(7, dtype=torch.float64, device=ws.device)
    L.check(L.lib().c2b_align_rotation_errors_rows(_p(x_cam15), _p(y_cam15), x_cam15.shape[0], C.byref(sim), _p(use), _p(err), _p(ws), _p(out), _stream()))
    return out


def similarity_apply(cam15, pts4, sim):
    """c2b_similarity_apply: cam15 [n, 15] and pts4 [n, 4] moved in place (either may be None)"""
    L.check(L.lib().c2b_similarity_apply(_p(cam15), cam15.shape[0] if cam15 is not None else 0, _p(pts4), pts4.shape[0] if pts4 is not None else 0,
                                         C.byref(sim), _stream()))


def stats_partial_pass1(camblk, cam_base, n_cam_global, pts4_slice, pt_base, n_entities_global, ws, part=None, centers=None):
    """this shard's share of the statistics (c2b_stats_partial_pass1); pts4_slice = the rows of the point table this
    rank reduces"""
    part = part if part is not None else torch.empty(L.STATS_DOUBLES, dtype=torch.float64, device=camblk.device)
    L.check(L.lib().c2b_stats_partial_pass1(_p(camblk), _pn(centers, camblk.shape[0]), camblk.shape[0], int(cam_base), int(n_cam_global), _p(pts4_slice),
                                            pts4_slice.shape[0], int(pt_base), int(n_entities_global), _p(ws), _p(part),
                                            _stream()))
    return part


def stats_partial_pass2(camblk, pts4_slice, mean3, ws, out=None, centers=None):
    out = out if out is not None else torch.empty(3, dtype=torch.float64, device=camblk.device)
    L.check(L.lib().c2b_stats_partial_pass2(_p(camblk), _pn(centers, camblk.shape[0]), camblk.shape[0], _p(pts4_slice), pts4_slice.shape[0], _p(mean3),
                                            _p(ws), _p(out), _stream()))
    return out


def add_drift_sharded(cam15, cam_base, pts4, stats_, strength, angle_strength, std, seed, direction=None):
    """direction None = add_drift_normalized (src/noise.rs:47-56), else add_drift with that direction"""
    d = (0.0, 0.0, 0.0) if direction is None else [float(x) for x in direction]
    L.check(L.lib().c2b_add_drift_sharded(_p(cam15), cam15.shape[0], int(cam_base), _p(pts4), pts4.shape[0], _p(stats_),
                                          1 if direction is None else 0, float(strength), float(angle_strength),
                                          float(std), d[0], d[1], d[2], int(seed), _stream()))


def add_noise_entities_sharded(cam15, cam_base, pts4, stats_, translation_std, rotation_std, point_std, seed):
    L.check(L.lib().c2b_add_noise_entities_sharded(_p(cam15), cam15.shape[0], int(cam_base), _p(pts4), pts4.shape[0],
                                                   _p(stats_), float(translation_std), float(rotation_std),
                                                   float(point_std), int(seed), _stream()))


def add_drift_normalized(cam15, pts4, stats_, strength, angle_strength, std, seed):
    L.check(L.lib().c2b_add_drift_normalized(_p(cam15), cam15.shape[0], _p(pts4), pts4.shape[0], _p(stats_),
                                             float(strength), float(angle_strength), float(std), int(seed), _stream()))


def add_noise_entities(cam15, pts4, stats_, translation_std, rotation_std, point_std, seed):
    L.check(L.lib().c2b_add_noise_entities(_p(cam15), cam15.shape[0], _p(pts4), pts4.shape[0], _p(stats_),
                                           float(translation_std), float(rotation_std), float(point_std), int(seed),
                                           _stream()))


def add_noise_observations(uv, obs_base, observations_std, seed):
    L.check(L.lib().c2b_add_noise_observations(_p(uv), uv.shape[0], int(obs_base), float(observations_std),
                                               int(seed), _stream()))


# ---- f32 extension (BASELINE configs[4]): the same entity kernels over a float state ---------------------
def to_f32(t):
    _chk(t, torch.float64, "to_f32 input")
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    L.check(L.lib().c2b_convert_f64_to_f32(_p(t), t.numel(), _p(out), _stream()))
    return out


def to_f64(t):
    _chk(t, torch.float32, "to_f64 input")
    out = torch.empty(t.shape, dtype=torch.float64, device=t.device)
    L.check(L.lib().c2b_convert_f32_to_f64(_p(t), t.numel(), _p(out), _stream()))
    return out


def stats_f32(cam15_f32, pts4_f32, ws, out=None):
    out = out if out is not None else torch.empty(L.STATS_DOUBLES, dtype=torch.float64, device=cam15_f32.device)
    L.check(L.lib().c2b_stats_f32(_p(cam15_f32), cam15_f32.shape[0], _p(pts4_f32), pts4_f32.shape[0], _p(ws), _p(out),
                                  _stream()))
    return out


def add_drift_f32(cam15, pts4, stats_, strength, angle_strength, std, dir_, seed):
    L.check(L.lib().c2b_add_drift_f32(_p(cam15), cam15.shape[0], _p(pts4), pts4.shape[0],
                                      C.c_void_p(stats_.data_ptr() + 15 * 8), float(strength), float(angle_strength),
                                      float(std), float(dir_[0]), float(dir_[1]), float(dir_[2]), int(seed), _stream()))


def add_drift_normalized_f32(cam15, pts4, stats_, strength, angle_strength, std, seed):
    L.check(L.lib().c2b_add_drift_normalized_f32(_p(cam15), cam15.shape[0], _p(pts4), pts4.shape[0], _p(stats_),
                                                 float(strength), float(angle_strength), float(std), int(seed),
                                                 _stream()))


def add_noise_entities_f32(cam15, pts4, stats_, translation_std, rotation_std, point_std, seed):
    L.check(L.lib().c2b_add_noise_entities_f32(_p(cam15), cam15.shape[0], _p(pts4), pts4.shape[0], _p(stats_),
                                               float(translation_std), float(rotation_std), float(point_std),
                                               int(seed), _stream()))


def add_sin_noise_f32(cam15, pts4, stats_, dir_, noise_dir, strength, frequency):
    L.check(L.lib().c2b_add_sin_noise_f32(_p(cam15), cam15.shape[0], _p(pts4), pts4.shape[0], _p(stats_),
                                          float(dir_[0]), float(dir_[1]), float(dir_[2]), float(noise_dir[0]),
                                          float(noise_dir[1]), float(noise_dir[2]), float(strength), float(frequency),
                                          _stream()))


# ---- the remaining Camera trait methods, batched (src/baproblem.rs:141-143, 165-175) ------------------------
def project_world(cam15, cam_idx, p3):
    out = torch.empty_like(p3)
    L.check(L.lib().c2b_project_world(_p(cam15), _p(cam_idx), _p(p3), p3.shape[0], _p(out), _stream()))
    return out


def to_world(cam15, cam_idx, p3):
    out = torch.empty_like(p3)
    L.check(L.lib().c2b_to_world(_p(cam15), _p(cam_idx), _p(p3), p3.shape[0], _p(out), _stream()))
    return out


def cameras_transform(cam15, delta_dir9, delta_loc3):
    L.check(L.lib().c2b_cameras_transform(_p(cam15), _p(delta_dir9), _p(delta_loc3), cam15.shape[0], _stream()))
    return cam15
