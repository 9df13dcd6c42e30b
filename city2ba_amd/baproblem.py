"""Host-side mirror of the reference's BAProblem<SnavelyCamera> for the hot path, over the C ABI.

Names, argument meaning and failure behaviour follow src/baproblem.rs (methods) and src/noise.rs
(free functions taking and returning a problem).  All arithmetic runs in the HIP library; this
file only moves numpy buffers across the boundary.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class ProblemOptions(C.Structure):
    """c2b_problem_options (include/city2ba_hip.h): which of two equivalent routes a problem's calls take and how many
    host threads they may use -- arguments of the C ABI, not environment variables"""
    _fields_ = [("host_text", C.c_int32), ("text_device_strict", C.c_int32), ("read_threads", C.c_int32), ("io_threads", C.c_int32),
                ("rank_sort_max_row", C.c_int32), ("reserved", C.c_int32), ("text_device_min_bytes", C.c_int64)]


_OPTION_NAMES = ("host_text", "text_device_strict", "read_threads", "io_threads", "rank_sort_max_row", "text_device_min_bytes")
_new_problem_options = {}        # what set_default_options changed: applied to every BAProblem made afterwards


def set_default_options(**kw):
    """options every BAProblem made from now on starts with (BAProblem.set_options changes one problem).  The classmethod
    constructors read files before a caller can reach the new object, so tests choose the parser this way.
    host_text, text_device_strict: bool; read_threads, io_threads, rank_sort_max_row: 0 = the library's default;
    text_device_min_bytes: -1 = the library's default (65 536)."""
    for k in kw:
        if k not in _OPTION_NAMES:
            raise TypeError("unknown option %r (one of %s)" % (k, ", ".join(_OPTION_NAMES)))
    _new_problem_options.update(kw)


def reset_default_options():
    _new_problem_options.clear()


def set_host_io_threads(n):
    """c2b_host_set_io_threads: threads of the host text formatter / parser for read_bal / write_bal and for problems
    whose options leave io_threads at 0 (n < 1: the library's default -- the usable cores, at most 16)"""
    L.lib().c2b_host_set_io_threads(int(n))


class BAProblem:
    """cameras + points + vis_graph (CSR) resident on one MI355X.

    `vis_graph` is the flattening of Vec<Vec<(usize,(f64,f64))>> (src/baproblem.rs:256-260):
    row_ptr[n_cam+1], pt_idx[n_obs], uv[n_obs,2], camera-major, in-camera order preserved."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self._device = int(device)
        L.check(L.lib().c2b_problem_create(int(device), C.byref(self._h)))
        self._row_ptr = np.zeros(1, dtype=np.uint64)
        self._pt_idx = np.zeros(0, dtype=np.uint64)
        if _new_problem_options:
            self.set_options(**_new_problem_options)

    def options(self):
        """this problem's c2b_problem_options as a dict"""
        o = ProblemOptions()
        L.check(L.lib().c2b_problem_get_options(self._h, C.byref(o)))
        return {k: getattr(o, k) for k in _OPTION_NAMES}

    def set_options(self, **kw):
        """c2b_problem_set_options: change the named options of this problem (see set_default_options for the names)"""
        o = ProblemOptions()
        L.check(L.lib().c2b_problem_get_options(self._h, C.byref(o)))
        for k, v in kw.items():
            if k not in _OPTION_NAMES:
                raise TypeError("unknown option %r (one of %s)" % (k, ", ".join(_OPTION_NAMES)))
            setattr(o, k, int(v))
        L.check(L.lib().c2b_problem_set_options(self._h, C.byref(o)))
        return self

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.lib().c2b_problem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- constructors -------------------------------------------------------------------
    @classmethod
    def from_visibility(cls, cams15, points, row_ptr, pt_idx, uv, device=0):
        """BAProblem::from_visibility (src/baproblem.rs:360-376); cameras as in-memory
        SnavelyCamera records [n,15] (R col-major, t, intrin)."""
        self = cls(device)
        self._upload(_f64(cams15, (-1, 15)), False, points, row_ptr, pt_idx, uv)
        return self

    @classmethod
    def from_bal(cls, bal9, points, row_ptr, pt_idx, uv, device=0):
        """Same with cameras as the 9-vectors a .bal/.bbal file holds (src/baproblem.rs:605-608)."""
        self = cls(device)
        self._upload(_f64(bal9, (-1, 9)), True, points, row_ptr, pt_idx, uv)
        return self

    @classmethod
    def new(cls, bal9, points, obs, device=0):
        """BAProblem::new (src/baproblem.rs:342-355): obs = iterable of (cam, point, u, v)."""
        bal9 = _f64(bal9, (-1, 9))
        points = _f64(points, (-1, 3))
        obs = list(obs)
        n_cam = len(bal9)
        for (ci, pi, _, _) in obs:
            if not (0 <= ci < n_cam):       # assert!(cam_i < cams.len())
                raise L.City2baError(L.ERR_INDEX_OUT_OF_RANGE, "camera index %d out of range" % ci)
            if not (0 <= pi < len(points)):  # assert!(p_i < points.len())
                raise L.City2baError(L.ERR_INDEX_OUT_OF_RANGE, "point index %d out of range" % pi)
        order = sorted(range(len(obs)), key=lambda k: obs[k][0])     # stable: keeps push order
        counts = np.bincount([obs[k][0] for k in order], minlength=n_cam) if obs else np.zeros(n_cam, int)
        row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        pt_idx = np.array([obs[k][1] for k in order], dtype=np.uint64)
        uv = np.array([[obs[k][2], obs[k][3]] for k in order], dtype=np.float64).reshape(-1, 2)
        return cls.from_bal(bal9, points, row_ptr, pt_idx, uv, device)

    def _upload(self, cams, is_bal, points, row_ptr, pt_idx, uv):
        points = _f64(points, (-1, 3))
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        pt_idx = np.ascontiguousarray(pt_idx, dtype=np.uint64)
        uv = _f64(uv, (-1, 2))
        if len(row_ptr) != len(cams) + 1:          # assert!(cams.len() == obs.len())
            raise L.City2baError(L.ERR_INVALID_ARGUMENT, "row_ptr must have n_cameras + 1 entries")
        if len(pt_idx) != len(uv) or (len(row_ptr) and int(row_ptr[-1]) != len(pt_idx)):
            raise L.City2baError(L.ERR_INVALID_ARGUMENT, "row_ptr[-1], pt_idx and uv disagree on n_obs")
        fn = L.lib().c2b_problem_upload_bal if is_bal else L.lib().c2b_problem_upload
        L.check(fn(self._h, len(cams), _ptr(cams), len(points), _ptr(points), _ptr(row_ptr), _ptr(pt_idx), _ptr(uv)))
        self._row_ptr, self._pt_idx = row_ptr, pt_idx

    # ---- counters (src/baproblem.rs:378-390) --------------------------------------------------
    def _sizes(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib().c2b_problem_sizes(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def num_cameras(self):
        return self._sizes()[0]

    def num_points(self):
        return self._sizes()[1]

    def num_observations(self):
        return self._sizes()[2]

    def __str__(self):   # Display, src/baproblem.rs:788-801
        return "Bundle Adjustment Problem with %d cameras, %d points, and %d observations" % self._sizes()

    # ---- data access -----------------------------------------------------------------------------
    @property
    def row_ptr(self):
        return self._row_ptr

    @property
    def pt_idx(self):
        return self._pt_idx

    def cameras(self):
        """in-memory SnavelyCamera records [n,15]"""
        out = np.empty((self.num_cameras(), 15))
        L.check(L.lib().c2b_problem_download(self._h, _ptr(out), None, None))
        return out

    def cameras_bal(self):
        """SnavelyCamera::to_vec for every camera [n,9] (src/baproblem.rs:189-202)"""
        out = np.empty((self.num_cameras(), 9))
        L.check(L.lib().c2b_problem_download_bal(self._h, _ptr(out)))
        return out

    def points(self):
        out = np.empty((self.num_points(), 3))
        L.check(L.lib().c2b_problem_download(self._h, None, _ptr(out), None))
        return out

    def observations(self):
        out = np.empty((self.num_observations(), 2))
        L.check(L.lib().c2b_problem_download(self._h, None, None, _ptr(out)))
        return out

    # ---- hot path ------------------------------------------------------------------------------------
    def project(self):
        """camera.project(camera.project_world(point)) for every observation (src/baproblem.rs:272)."""
        out = np.empty((self.num_observations(), 2))
        L.check(L.lib().c2b_problem_project(self._h, _ptr(out)))
        return out

    def total_reprojection_error(self, norm):
        """src/baproblem.rs:265-279"""
        out = C.c_double()
        L.check(L.lib().c2b_problem_total_reprojection_error(self._h, float(norm), C.byref(out)))
        return out.value

    def total_reprojection_errors_l1_l2(self):
        """(total_reprojection_error(1.), total_reprojection_error(2.)) from ONE pass over the observations -- the pair
        run_noise prints before and after the noise (src/bin/city2ba.rs:283-287, 350-354)"""
        l1, l2 = C.c_double(), C.c_double()
        L.check(L.lib().c2b_problem_total_reprojection_errors_l1_l2(self._h, C.byref(l1), C.byref(l2)))
        return l1.value, l2.value

    def residual_jacobian(self, out=None, pinned=False):
        """r [n,2], Jc [n,2,9] (w t f k1 k2 columns), Jp [n,2,3].  Build-defined: the reference has no Jacobian.
        out = (r, Jc, Jp) reuses the caller's arrays; pinned=True returns arrays in page-locked memory
        (pinned_empty), which receive the results at PCIe speed -- keep them and pass them back as `out` when
        calling repeatedly."""
        n = self.num_observations()
        if out is not None:
            r, Jc, Jp = out
            for a, shape in ((r, (n, 2)), (Jc, (n, 2, 9)), (Jp, (n, 2, 3))):
                if a.dtype != np.float64 or a.shape != shape or not a.flags.c_contiguous:
                    raise L.City2baError(L.ERR_INVALID_ARGUMENT, "residual_jacobian: out arrays must be C-contiguous float64 of shapes (n,2), (n,2,9), (n,2,3)")
        elif pinned:
            r, Jc, Jp = pinned_empty((n, 2)), pinned_empty((n, 2, 9)), pinned_empty((n, 2, 3))
        else:
            r, Jc, Jp = np.empty((n, 2)), np.empty((n, 2, 9)), np.empty((n, 2, 3))
        L.check(L.lib().c2b_problem_residual_jacobian(self._h, _ptr(r), _ptr(Jc), _ptr(Jp)))
        return r, Jc, Jp

    def residual_jacobian_device(self, outputs=None, max_attempts=8):
        """residual + Jacobian of every observation in ONE launch with the results left on the device
        (c2b_problem_residual_jacobian_device): returns (outputs, sum_sq) -- outputs.r [n,2], .Jc [n,18], .Jp [n,6] are
        torch views of device arrays placed for streaming stores (device.JacobianOutputs; pass the object back in to
        reuse it in a loop), sum_sq = sum of squared residuals (total_reprojection_error(2.) ** 2).  The BAProblem-level
        route to the Level-0 headline rate: nothing but the 8-byte sum crosses PCIe."""
        from . import device as D
        h = C.c_void_p(outputs.handle.value) if outputs is not None else C.c_void_p()
        s = C.c_double()
        L.check(L.lib().c2b_problem_residual_jacobian_device(self._h, int(max_attempts), C.byref(h), C.byref(s)))
        if outputs is None:
            outputs = D.JacobianOutputs(self.num_observations(), self._device, max_attempts, _handle=h)
        return outputs, s.value

    def normal_equations(self, out=None):
        """The Gauss-Newton diagonal blocks and gradient, reduced on the device from the Jacobian residual_jacobian
        returns (c2b_problem_normal_equations): (U [n_cam,9,9], gc [n_cam,9], V [n_pts,3,3], gp [n_pts,3], sum_sq) --
        U = sum Jc^T Jc and gc = sum Jc^T r per camera, V = sum Jp^T Jp and gp = sum Jp^T r per point, sum_sq = sum |r|^2.
        The four arrays are float64 torch tensors on the problem's device; out = (U, gc, V, gp) fills the caller's
        (contiguous float64 on that device, of those shapes; an entry of None skips its pass together with its partner,
        which must be None too).  Deterministic: the same problem gives the same bits on every call.  On a shard U / gc
        are the shard's cameras and V / gp its partial sums over its own observations (they add up over the ranks)."""
        import torch
        nc, npt = self.num_cameras(), self.num_points()
        dev = torch.device("cuda", self._device)
        shapes = ((nc, 9, 9), (nc, 9), (npt, 3, 3), (npt, 3))
        if out is None:
            arrs = [torch.empty(sh, dtype=torch.float64, device=dev) for sh in shapes]
        else:
            arrs = list(out)
            if len(arrs) != 4:
                raise ValueError("normal_equations: out must be (U, gc, V, gp)")
            for a, sh, name in zip(arrs, shapes, ("U", "gc", "V", "gp")):
                if a is None:
                    continue
                if not isinstance(a, torch.Tensor) or a.dtype != torch.float64 or a.device != dev or tuple(a.shape) != sh \
                        or not a.is_contiguous():
                    raise ValueError("normal_equations: out %s must be a contiguous float64 tensor of shape %s on %s" % (name, sh, dev))
            if (arrs[0] is None) != (arrs[1] is None) or (arrs[2] is None) != (arrs[3] is None):
                raise ValueError("normal_equations: U / gc and V / gp are given or skipped in pairs")
        s = C.c_double()
        ptr = lambda a: C.c_void_p(a.data_ptr()) if a is not None and a.numel() else None     # empty: no pass to run
        U, gc, V, gp = arrs
        # the library's stream is its own: work queued on torch's stream for these tensors must be done first
        torch.cuda.current_stream(dev).synchronize()
        L.check(L.lib().c2b_problem_normal_equations(self._h, ptr(U), ptr(gc), ptr(V), ptr(gp), C.byref(s)))
        return U, gc, V, gp, s.value

    def set_loss(self, kind, scale=1.0):
        """The robust loss of normal_equations / solve_step / robust_cost (c2b_problem_set_loss): "huber", "cauchy" or
        "soft_l1" with its scale a > 0 (Ceres' definitions, in the units of the residuals), or None for the squared loss.
        Under a loss the step is one of iteratively reweighted least squares: every observation's (r, Jc, Jp) is scaled by
        sqrt(w), w = rho'(|r|^2) at the current state; sum_sq and model_decrease are then the weighted quantities, and
        robust_cost() is what a loop minimises.  The loss belongs to the handle: uploads and culls keep it."""
        L.check(L.lib().c2b_problem_set_loss(self._h, L.loss_kind(kind), float(scale)))

    @property
    def loss(self):
        """(name, scale) of the loss in force; (None, 1.0) is the squared loss"""
        k, a = C.c_int(), C.c_double()
        L.check(L.lib().c2b_problem_get_loss(self._h, C.byref(k), C.byref(a)))
        return L.LOSS_NAMES[k.value], a.value

    def robust_cost(self):
        """sum rho(|r|^2) over the observations under the problem's loss, on the device (c2b_problem_robust_cost); with
        the squared loss, sum |r|^2"""
        s = C.c_double()
        L.check(L.lib().c2b_problem_robust_cost(self._h, C.byref(s)))
        return s.value

    def set_preconditioner(self, kind):
        """What solve_step's PCG is preconditioned with (c2b_problem_set_preconditioner): "block_jacobi", the 9x9 blocks
        of the damped U (the default), or "schur_jacobi", the 9x9 diagonal blocks of the Schur complement itself -- one
        more pass over the observations in the set-up and the same kernels per iteration; it changes the iteration
        count, not the solution (measurements: DESIGN 4.4).  The setting belongs to the handle: uploads and culls keep it."""
        L.check(L.lib().c2b_problem_set_preconditioner(self._h, L.precond_kind(kind)))

    @property
    def preconditioner(self):
        """the name of the preconditioner in force"""
        k = C.c_int()
        L.check(L.lib().c2b_problem_get_preconditioner(self._h, C.byref(k)))
        return L.PRECOND_NAMES[k.value]

    def preconditioner_fallbacks(self):
        """cameras whose Schur-Jacobi block could not be factored in the last solve_step and took the block-Jacobi
        factor instead (c2b_problem_preconditioner_fallbacks); 0 after a block-Jacobi solve"""
        n = C.c_int64()
        L.check(L.lib().c2b_problem_preconditioner_fallbacks(self._h, C.byref(n)))
        return n.value

    def set_schur(self, kind):
        """How solve_step applies the reduced camera system S (c2b_problem_set_schur): "implicit", two passes over
        the observations per PCG iteration and S never formed (the default), or "explicit", S formed once per step in
        block-CSR on the covisibility pattern and one product with the stored blocks per iteration -- an iteration then
        costs edges, not observations, at the price of the build and of schur_bytes() of device memory.  It changes the
        arithmetic of the iteration, not what the step converges to.  The setting belongs to the handle: uploads and culls
        keep it, window() and subset(carry=True) carry it.  If the blocks cannot be allocated solve_step raises with the
        bytes in the message; there is no fallback, and the handle stays usable under "implicit"."""
        L.check(L.lib().c2b_problem_set_schur(self._h, L.schur_kind(kind)))

    def schur(self):
        """the name of the setting in force: "implicit" or "explicit" """
        k = C.c_int()
        L.check(L.lib().c2b_problem_get_schur(self._h, C.byref(k)))
        return L.SCHUR_NAMES[k.value]

    def schur_bytes(self):
        """device bytes the explicit setting adds to the solve buffers, 648 (n_edges + n_cam) + 216 n_obs
        (c2b_problem_schur_bytes); builds the pattern"""
        n = C.c_int64()
        L.check(L.lib().c2b_problem_schur_bytes(self._h, C.byref(n)))
        return n.value

    def set_linear_solver(self, kind):
        """How solve_step solves the reduced camera system S dc = b (c2b_problem_set_linear_solver): "pcg", the
        preconditioned conjugate gradients (the default), or "cholesky": S formed as the explicit setting forms it whatever
        set_schur says, scattered into a dense lower triangle, factored by a blocked Cholesky on the device and solved by two
        substitutions -- the exact step, 0 iterations, no max_iters or rel_tol to choose, at linear_solver_bytes() of device
        memory; for the few hundred cameras of a window, not for a whole city (at most 4096 cameras).  A factor that fails
        (a pivot not finite or <= 0) gives status 2 and a zero step, which the LM loops answer by raising the damping.  The
        setting belongs to the handle: uploads and culls keep it, window() and subset(carry=True) carry it.  If the buffers
        cannot be allocated solve_step raises with the bytes in the message; there is no fallback, and the handle stays
        usable under "pcg"."""
        L.check(L.lib().c2b_problem_set_linear_solver(self._h, L.linear_kind(kind)))

    def linear_solver(self):
        """the name of the linear solver in force: "pcg" or "cholesky" """
        k = C.c_int()
        L.check(L.lib().c2b_problem_get_linear_solver(self._h, C.byref(k)))
        return L.LINEAR_NAMES[k.value]

    def linear_solver_bytes(self):
        """device bytes the "cholesky" setting adds to the solve buffers: schur_bytes() + 8 (Np^2 + 2 Np), Np = 64 ceil(9 n_cam / 64)
        (c2b_problem_linear_solver_bytes); builds the pattern; refused above 4096 cameras"""
        n = C.c_int64()
        L.check(L.lib().c2b_problem_linear_solver_bytes(self._h, C.byref(n)))
        return n.value

    def schur_complement(self, lam):
        """The reduced camera system at damping lam, built on the device (c2b_problem_schur_complement) under the handle's loss,
        masks and priors, whatever set_schur says: (nbr_ptr [n_cam + 1] uint64, nbr [n_edges] uint32, S_diag [n_cam, 9, 9],
        S_off [n_edges, 9, 9], b [n_cam, 9]) as numpy arrays.  Row c of S holds S_diag[c] on the diagonal and S_off[e] in block
        column nbr[e] for e in [nbr_ptr[c], nbr_ptr[c + 1]): the covisibility graph at min_shared = 1, both triangles stored,
        S_off of (c', c) the transpose of (c, c') bit for bit.  S dc = b is the system solve_step solves.  The call needs
        schur_bytes() of device memory besides the arrays it returns; under "implicit" that is freed again before it returns."""
        import torch
        nc = self.num_cameras()
        nbr_ptr = np.zeros(nc + 1, dtype=np.uint64)
        L.check(L.lib().c2b_problem_get_schur_pattern(self._h, _ptr(nbr_ptr), None))
        ne = int(nbr_ptr[-1])
        nbr = np.zeros(ne, dtype=np.uint32)
        if ne:
            L.check(L.lib().c2b_problem_get_schur_pattern(self._h, None, _ptr(nbr)))
        dev = torch.device("cuda", self._device)
        f64 = dict(dtype=torch.float64, device=dev)
        Sd, So, b = torch.empty((nc, 9, 9), **f64), torch.empty((ne, 9, 9), **f64), torch.empty((nc, 9), **f64)
        ptr = lambda a: C.c_void_p(a.data_ptr()) if a.numel() else None
        n = C.c_int64()
        torch.cuda.current_stream(dev).synchronize()
        # (an empty tensor has no address: a problem without cameras passes a dummy the library never writes through)
        dummy = torch.empty(1, **f64)
        L.check(L.lib().c2b_problem_schur_complement(self._h, float(lam), ptr(Sd) or ptr(dummy), ptr(So), ptr(b) or ptr(dummy), C.byref(n)))
        assert n.value == ne
        return nbr_ptr, nbr, Sd.cpu().numpy(), So.cpu().numpy(), b.cpu().numpy()

    def set_constant(self, cameras=None, points=None):
        """Hold camera parameters and points constant in normal_equations / solve_step / apply_step
        (c2b_problem_set_constant).  cameras: uint16 [n_cam], bit k set = parameter k constant, k in to_vec order
        (ω0 ω1 ω2 t0 t1 t2 f k1 k2; solve.ROTATION ... solve.ALL name the groups), or bool [n_cam, 9]; points: bool [n_pts].
        None: none of that kind; both None clears the masks.  The step is that of the problem in which the constant
        parameters cannot move, their entries of dc / dp are exactly 0, and apply_step leaves them bit for bit.  The
        masks belong to the handle: they survive apply_step, noise and an upload of the same counts, and are dropped by
        whatever changes a count or renumbers the entities (cull, read, the generators)."""
        nc, npt = self.num_cameras(), self.num_points()
        cm = pm = None
        if cameras is not None:
            a = np.asarray(cameras)
            if a.dtype == np.bool_:
                if a.shape != (nc, 9):
                    raise ValueError("set_constant: a bool cameras mask must have shape (%d, 9)" % nc)
                cm = np.ascontiguousarray((a.astype(np.uint16) << np.arange(9, dtype=np.uint16)).sum(axis=1, dtype=np.uint16))
            else:
                if a.shape != (nc,) or not np.issubdtype(a.dtype, np.integer) or (a.size and (a.min() < 0 or a.max() > 0xffff)):
                    raise ValueError("set_constant: cameras must be uint16 [%d] or bool [%d, 9]" % (nc, nc))
                cm = np.ascontiguousarray(a, dtype=np.uint16)
        if points is not None:
            a = np.asarray(points)
            if a.shape != (npt,) or not (a.dtype == np.bool_ or np.issubdtype(a.dtype, np.integer)) or \
                    (a.size and (a.min() < 0 or a.max() > 0xff)):
                raise ValueError("set_constant: points must be bool [%d]" % npt)
            pm = np.ascontiguousarray(a, dtype=np.uint8)
        L.check(L.lib().c2b_problem_set_constant(self._h, _ptr(cm), _ptr(pm)))

    def constant(self):
        """the masks in force (c2b_problem_get_constant): (bool [n_cam, 9], bool [n_pts]); all False when none is set"""
        cm = np.zeros(self.num_cameras(), dtype=np.uint16)
        pm = np.zeros(self.num_points(), dtype=np.uint8)
        L.check(L.lib().c2b_problem_get_constant(self._h, _ptr(cm), _ptr(pm), None, None))
        return ((cm[:, None] >> np.arange(9, dtype=np.uint16)) & 1).astype(bool), pm.astype(bool)

    def set_priors(self, camera_centers=None, camera_center_weights=None, intrinsics=None, intrinsics_weights=None, points=None,
                   point_weights=None):
        """Soft constraints beside the observations in normal_equations / solve_step / the LM loops (c2b_problem_set_priors):
        r_C = w_C o (C - C0) on the cameras' world-frame centres, r_I = w_I o ((f, k1, k2) - I0) on their intrinsics and
        r_X = w_X o (X - X0) on the points; the cost gains sum |r_prior|^2.  Each kind is a target [n, 3] and weights
        [n, 3] >= 0 (1 / sigma in units of the observations' standard deviation; 0 switches a row off; a scalar or a
        length-3 weight broadcasts over the rows).  A target left None under a given weight is the problem's current
        value; a kind whose weight is None has no prior, and all None clears the priors.  No robust loss reweights a prior.
        The priors belong to the handle exactly as the constant masks do: kept by apply_step, noise and an upload of the
        same counts, dropped by whatever changes a count or renumbers the entities."""
        nc, npt = self.num_cameras(), self.num_points()

        def pair(target, w, n, current, name):
            if w is None:
                if target is not None:
                    raise ValueError("set_priors: %s given without weights" % name)
                return None, None
            w = np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.float64), (n, 3)))
            t = current() if target is None else _f64(target, (-1, 3))
            if t.shape != (n, 3):
                raise ValueError("set_priors: %s must have shape (%d, 3)" % (name, n))
            return np.ascontiguousarray(t), w
        c0, cw = pair(camera_centers, camera_center_weights, nc, self._camera_centers, "camera_centers")
        i0, iw = pair(intrinsics, intrinsics_weights, nc, lambda: self.cameras_bal()[:, 6:9].copy(), "intrinsics")
        x0, xw = pair(points, point_weights, npt, self.points, "points")
        L.check(L.lib().c2b_problem_set_priors(self._h, _ptr(c0), _ptr(cw), _ptr(i0), _ptr(iw), _ptr(x0), _ptr(xw)))

    @property
    def priors(self):
        """the priors in force (c2b_problem_get_priors): dict(camera_centers, camera_center_weights, intrinsics,
        intrinsics_weights, points, point_weights -- [n, 3] each, zeros for a kind with none --, active = (cameras with a
        centre row, cameras with an intrinsics row, points with a row) of positive weight)"""
        nc, npt = self.num_cameras(), self.num_points()
        a = [np.zeros((n, 3)) for n in (nc, nc, nc, nc, npt, npt)]
        k = [C.c_int64(), C.c_int64(), C.c_int64()]
        L.check(L.lib().c2b_problem_get_priors(self._h, *[_ptr(x) for x in a], *[C.byref(x) for x in k]))
        names = ("camera_centers", "camera_center_weights", "intrinsics", "intrinsics_weights", "points", "point_weights")
        out = dict(zip(names, a))
        out["active"] = tuple(x.value for x in k)
        return out

    def prior_cost(self):
        """sum |r_prior|^2 at the current state, on the device (c2b_problem_prior_cost); 0.0 without priors"""
        s = C.c_double()
        L.check(L.lib().c2b_problem_prior_cost(self._h, C.byref(s)))
        return s.value

    def prior_residual_jacobian(self):
        """(r_cam [n_cam, 6] = (r_C, r_I), A_cam [n_cam, 3, 6] = diag(w_C) [dC/dw | -R^T], r_pt [n_pts, 3]) of the priors in
        force (c2b_problem_prior_residual_jacobian); zeros where there is none.  The columns are those of residual_jacobian."""
        r, A, rp = np.empty((self.num_cameras(), 6)), np.empty((self.num_cameras(), 3, 6)), np.empty((self.num_points(), 3))
        L.check(L.lib().c2b_problem_prior_residual_jacobian(self._h, _ptr(r), _ptr(A), _ptr(rp)))
        return r, A, rp

    def solve_step(self, lam, max_iters=100, rel_tol=1e-6, out=None):
        """One damped Gauss-Newton (Levenberg-Marquardt) step on the device (c2b_problem_solve_step): the solution of
        (J^T J + lam D) delta = -g, D = diag(min(max(diag(J^T J), 1e-6), 1e32)), by PCG on the Schur complement of the
        cameras.  Returns (dc [n_cam,9], dp [n_pts,3], info): float64 torch tensors on the problem's device (out = (dc, dp)
        fills the caller's, contiguous float64 of those shapes) and info = dict(iterations, status -- 0 converged,
        1 max_iters, 2 breakdown --, rel_residual, sum_sq = |r|^2 now, model_decrease = |r|^2 - |r + J delta|^2).
        The columns of dc are those of residual_jacobian (the ω of this mode); apply_step adds the step."""
        import torch
        nc, npt = self.num_cameras(), self.num_points()
        dev = torch.device("cuda", self._device)
        shapes = ((nc, 9), (npt, 3))
        if out is None:
            arrs = [torch.empty(sh, dtype=torch.float64, device=dev) for sh in shapes]
        else:
            arrs = list(out)
            if len(arrs) != 2:
                raise ValueError("solve_step: out must be (dc, dp)")
            for a, sh, name in zip(arrs, shapes, ("dc", "dp")):
                if not isinstance(a, torch.Tensor) or a.dtype != torch.float64 or a.device != dev or tuple(a.shape) != sh \
                        or not a.is_contiguous():
                    raise ValueError("solve_step: out %s must be a contiguous float64 tensor of shape %s on %s" % (name, sh, dev))
        info = L.StepInfo()
        ptr = lambda a: C.c_void_p(a.data_ptr()) if a.numel() else None
        torch.cuda.current_stream(dev).synchronize()
        L.check(L.lib().c2b_problem_solve_step(self._h, float(lam), int(max_iters), float(rel_tol), ptr(arrs[0]), ptr(arrs[1]),
                                               C.byref(info)))
        d = {k: getattr(info, k) for k, _ in L.StepInfo._fields_}
        return arrs[0], arrs[1], d

    def apply_step(self, dc, dp):
        """cameras and points += a step of solve_step (c2b_problem_apply_step): bal9 = to_vec of the cameras + dc, the
        cameras rebuilt from it, points + dp; either may be None (no change).  The problem is in bal mode afterwards."""
        import torch
        dev = torch.device("cuda", self._device)
        for a, sh, name in ((dc, (self.num_cameras(), 9), "dc"), (dp, (self.num_points(), 3), "dp")):
            if a is not None and (not isinstance(a, torch.Tensor) or a.dtype != torch.float64 or a.device != dev
                                  or tuple(a.shape) != sh or not a.is_contiguous()):
                raise ValueError("apply_step: %s must be a contiguous float64 tensor of shape %s on %s" % (name, sh, dev))
        ptr = lambda a: C.c_void_p(a.data_ptr()) if a is not None and a.numel() else None
        torch.cuda.current_stream(dev).synchronize()
        L.check(L.lib().c2b_problem_apply_step(self._h, ptr(dc), ptr(dp)))

    def checkpoint(self):
        """Keep the cameras and points as they are now, on the device (c2b_problem_checkpoint); the problem is in bal mode
        afterwards, as after apply_step(None, None).  rollback() returns to this state bit for bit.  apply_step and the
        noise functions leave the checkpoint in place; any upload, a cull, a read and the generators drop it."""
        L.check(L.lib().c2b_problem_checkpoint(self._h))

    def rollback(self):
        """Cameras and points back to the last checkpoint() (c2b_problem_rollback): two device-to-device copies; the row
        structure, the solve buffers, the loss, the preconditioner and the masks stay.  Raises without a checkpoint."""
        L.check(L.lib().c2b_problem_rollback(self._h))

    def drop_checkpoint(self):
        """Forget the checkpoint (c2b_problem_drop_checkpoint); rollback() raises until the next checkpoint()."""
        L.check(L.lib().c2b_problem_drop_checkpoint(self._h))

    def _stats(self):
        s = np.empty(L.STATS_DOUBLES)
        L.check(L.lib().c2b_problem_stats(self._h, _ptr(s)))
        return s

    def mean(self):          # src/baproblem.rs:282-289
        return self._stats()[0:3].copy()

    def std(self):           # src/baproblem.rs:292-304
        return self._stats()[3:6].copy()

    def extent(self):        # src/baproblem.rs:307-331
        s = self._stats()
        return s[6:9].copy(), s[9:12].copy()

    def dimensions(self):    # src/baproblem.rs:334-337
        return self._stats()[12:15].copy()

    def drift_origin(self):
        """element of centers ++ points closest to the world origin (src/noise.rs:75-87)"""
        s = self._stats()
        return s[15:18].copy(), int(s[18])

    def generate_world_points(self, triangles, num_points, max_dist, seed=0):
        """generate_world_points_uniform (src/generate.rs:356-420) for this problem's cameras, on the device: its points
        are replaced by `num_points` points sampled on the mesh by area, each within max_dist of some camera (the same
        points as generate.generate_world_points_uniform with the same seed).  The problem must hold no observations."""
        tri = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
        n = C.c_int64()
        L.check(L.lib().c2b_problem_generate_world_points(self._h, _ptr(tri), len(tri), int(num_points), float(max_dist),
                                                          int(seed), C.byref(n)))
        return n.value

    def visibility_graph(self, max_dist, triangles=None, fetch=True, prebuilt_hierarchy=False, dense=False):
        """generate::visibility_graph (src/generate.rs:424-481): for every camera the points within max_dist of its centre
        (`locate_within_distance`) that pass the predicate -- through the cell list of c2b_problem_visibility_within_distance,
        or, with dense=True, by the brute-force sweep of every camera against every point (the same lists: the sweep is
        what BASELINE's 1e10-pair configuration times); with `triangles` ([n,9] f32 mesh) the survivors also pass the
        occlusion rays of :455-476 (a hierarchy on the device in place of Embree).  Returns the CSR graph (row_ptr u64,
        pt_idx u64, uv) with points in ascending order per camera, like the reference's push order."""
        n_cam = self.num_cameras()
        row_ptr = np.zeros(n_cam + 1, dtype=np.uint64)
        if dense:
            L.check(L.lib().c2b_problem_visibility_dense(self._h, float(max_dist), _ptr(row_ptr)))
        else:
            L.check(L.lib().c2b_problem_visibility_within_distance(self._h, float(max_dist), 0, 0.0, 0.0, _ptr(row_ptr)))
        if triangles is not None:
            tri = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
            if prebuilt_hierarchy and len(tri):
                # the caller-built form (c2b_bvh_build needs only the triangles: cli/main.cpp builds it on a second
                # thread while cameras are placed and points sampled)
                h = C.c_void_p()
                L.check(L.lib().c2b_bvh_build(_ptr(tri), len(tri), C.byref(h)))
                try:
                    L.check(L.lib().c2b_problem_visibility_dense_occlude_bvh(self._h, h, _ptr(row_ptr)))
                finally:
                    L.lib().c2b_bvh_free(h)
            else:
                L.check(L.lib().c2b_problem_visibility_dense_occlude(self._h, _ptr(tri), len(tri), _ptr(row_ptr)))
        if not fetch:                     # lists stay on the device for adopt_visibility()
            return row_ptr
        n = int(row_ptr[-1])
        pt_idx = np.empty(n, dtype=np.uint64)
        uv = np.empty((n, 2))
        L.check(L.lib().c2b_problem_visibility_dense_fetch(self._h, _ptr(pt_idx), _ptr(uv)))
        return row_ptr, pt_idx, uv

    def _cameras_from_position_direction(self, pos, dirs):
        """Camera::from_position_direction (src/baproblem.rs:153-159), batched on this problem's device."""
        pos, dirs = _f64(pos, (-1, 3)), _f64(dirs, (-1, 9))
        out = np.empty((len(pos), 15))
        L.check(L.lib().c2b_problem_from_position_direction(self._h, len(pos), _ptr(pos), _ptr(dirs), _ptr(out)))
        return out

    def _camera_centers(self):
        """Camera::center (src/baproblem.rs:161-163) of every camera [n,3]"""
        out = np.empty((self.num_cameras(), 3))
        L.check(L.lib().c2b_problem_centers(self._h, _ptr(out)))
        return out

    # ---- host-side rows: cull and file IO (C++ host code behind the same ABI) -----------------------
    def cull(self, faithful=True):
        """BAProblem::cull (src/baproblem.rs:538-549): largest connected component + cameras with > 3
        observations / points with > 1, to a fixed point -- on the device, in place (the reference consumes self and
        returns the culled problem; this returns self)."""
        L.check(L.lib().c2b_problem_cull(self._h, int(bool(faithful))))
        return self._refresh_graph()

    def largest_connected_component(self, faithful=True):
        """BAProblem::largest_connected_component (src/baproblem.rs:456-534), one application, on the device"""
        L.check(L.lib().c2b_problem_largest_connected_component(self._h, int(bool(faithful))))
        return self._refresh_graph()

    def remove_singletons(self):
        """BAProblem::remove_singletons (src/baproblem.rs:426-453), one application, on the device"""
        L.check(L.lib().c2b_problem_remove_singletons(self._h))
        return self._refresh_graph()

    def filter_observations(self, max_error, in_front=False):
        """Outlier rejection in place, on the device (c2b_problem_filter_observations): every observation whose
        reprojection residual has |r|^2 > max_error^2, or is NaN, is dropped (max_error = inf drops the NaN ones alone), and with in_front=True
        every one whose point is not in front of its camera too.  The survivors keep their order inside every camera's
        list; cameras and points are not renumbered, so the constant masks, the loss, the preconditioner and a checkpoint
        stay.  Returns the number removed (0: nothing changed).  A filter can leave a camera or a point with too few
        observations: cull() is the caller's call."""
        n = C.c_int64()
        L.check(L.lib().c2b_problem_filter_observations(self._h, float(max_error), L.FILTER_IN_FRONT if in_front else 0, C.byref(n)))
        if n.value:
            self._refresh_graph()
        return n.value

    def merge_points(self, radius, max_error, rounds=1, return_map=False):
        """Duplicate landmarks merged in place, on the device (c2b_problem_merge_points): the repair of
        split_landmarks and of broken tracks.  Per round every observed point that is neither constant nor tied to a point
        prior picks the nearest other such point within `radius` that shares no camera with it and whose merged position
        -- between the two, weighted by their observation counts -- reprojects every observation of both within max_error
        in front of its camera (filter_observations' predicate with in_front); pairs that pick each other are merged onto
        the lower index.  Up to `rounds` rounds, each on the state the last one left; a round that merges nothing is the
        last.  Cameras and points are not renumbered and uv, the row pointer and the order inside every camera's list
        stay, so the constant masks, the priors, the loss, the preconditioner and a checkpoint stay too.  The absorbed
        points are NOT culled: they stay in the table as unobserved points (the LM step leaves them where they are);
        cull() is the caller's call.  Returns dict(merged, rounds): the number of points absorbed and of rounds run; with
        return_map also the int32 map [n_pts]: the point each point's observations ended on (itself when not absorbed)."""
        merged, run = C.c_int64(), C.c_int()
        into = np.zeros(self.num_points(), dtype=np.int32) if return_map else None
        L.check(L.lib().c2b_problem_merge_points(self._h, float(radius), float(max_error), int(rounds),
                                                 into.ctypes.data_as(C.c_void_p) if return_map else None, C.byref(merged), C.byref(run)))
        if merged.value:
            self._refresh_graph()
        out = dict(merged=int(merged.value), rounds=int(run.value))
        return (out, into) if return_map else out

    def rematch_observations(self, radius, max_error, min_fits=2, return_status=False):
        """Wrong matches relabelled in place, on the device (c2b_problem_rematch_observations): the repair of
        add_incorrect_correspondences and join_landmarks that keeps the measurement.  An observation that fits its point
        (filter_observations' predicate with in_front at max_error) stays; so does one whose point fewer than min_fits
        observations fit or that is not finite (skipped: nothing is judged about such a point, and nothing assigned to it).
        Every other observation gives its label up and takes the trusted point it fits best among the points within `radius`
        of the one it named and the labels the other failing observations of its camera gave up, unless an observation of
        that camera that stays already names it; of two observations of a camera that want one point the better fit gets it.
        Whoever is left without a point is removed, as the filter would remove it.  Cameras and points neither move nor are
        renumbered, the survivors keep their order and the bits of their pixels, and the constant masks, the priors, the
        loss, the preconditioner and a checkpoint stay.  Returns dict(fits, skipped, reassigned, removed); with
        return_status also the uint8 status [n_obs before the call] (_lib.REMATCH_STATUS order)."""
        status = np.zeros(self.num_observations(), dtype=np.uint8)
        reassigned, removed = C.c_int64(), C.c_int64()
        L.check(L.lib().c2b_problem_rematch_observations(self._h, float(radius), float(max_error), int(min_fits),
                                                         status.ctypes.data_as(C.c_void_p), C.byref(reassigned), C.byref(removed)))
        if reassigned.value or removed.value:
            self._refresh_graph()
        out = dict(zip(L.REMATCH_STATUS, (int(v) for v in np.bincount(status, minlength=4))))
        assert (out["reassigned"], out["removed"]) == (reassigned.value, removed.value)
        return (out, status) if return_status else out

    # ---- index noise in place: a second, counter-based draw scheme next to noise.py's host route ----
    def _index_noise(self, entry, value, seed):
        n = C.c_int64()
        L.check(entry(self._h, float(value), int(seed), C.byref(n)))
        if n.value:
            self._refresh_graph()
        return n.value

    def drop_features(self, keep_fraction, seed=0):
        """drop_features (src/noise.rs:229-251) in place, on the device: every camera keeps floor(len * keep_fraction) of its
        observations, those with the smallest (draw, index); the survivors keep their order.  Masks, priors, loss and options
        stay as across filter_observations.  Returns the number removed."""
        return self._index_noise(L.lib().c2b_problem_drop_features, keep_fraction, seed)

    def add_incorrect_correspondences(self, mismatch_chance, seed=0):
        """add_incorrect_correspondences (src/noise.rs:180-226) in place, on the device: the pixels stay, point indices are
        swapped inside a camera.  Returns the number of observations that swapped (one with itself included)."""
        return self._index_noise(L.lib().c2b_problem_add_incorrect_correspondences, mismatch_chance, seed)

    def split_landmarks(self, split_fraction, seed=0):
        """split_landmarks (src/noise.rs:255-291) in place, on the device: floor(split_fraction * n_pts) points are
        duplicated at the table's end and half of their observations move to the copy.  The point count changes: masks,
        priors, a checkpoint and an origin are dropped as cull drops them.  Returns the number of points duplicated."""
        return self._index_noise(L.lib().c2b_problem_split_landmarks, split_fraction, seed)

    def join_landmarks(self, join_fraction, seed=0):
        """join_landmarks (src/noise.rs:323-378) in place, on the device: floor(join_fraction * n_pts) observations take
        one of the ten nearest other points of their point.  Returns the number of observations relabelled."""
        return self._index_noise(L.lib().c2b_problem_join_landmarks, join_fraction, seed)

    def _status_pass(self, entry, args, n, names, return_status):
        """entry(handle, *args, status, counts) over n entities: the counts as a dict under `names`, and the status bytes"""
        counts = np.zeros(len(names), dtype=np.int64)
        status = np.zeros(n, dtype=np.uint8) if return_status else None
        L.check(entry(self._h, *args, status.ctypes.data_as(C.c_void_p) if return_status else None, counts.ctypes.data_as(C.c_void_p)))
        out = dict(zip(names, (int(v) for v in counts)))
        return (out, status) if return_status else out

    def triangulate_points(self, min_angle_deg=1.0, return_status=False):
        """Linear midpoint triangulation on the device (c2b_problem_triangulate_points): every point is set to
        the position nearest, in the sum of squared distances, to the rays of its observations through the cameras as
        they are -- a start for a solve, not a refinement.  A point keeps its bits when it is constant, has fewer than two
        usable observations, has rays less than min_angle_deg apart (the parallax test), or would lie behind one of its
        cameras.  The loss on the handle is ignored; masks, loss, preconditioner and a checkpoint stay.  Returns
        dict(triangulated, too_few, degenerate, behind, constant), the number of points of each outcome, and with
        return_status also the uint8 status per point (the dict's order: 0 .. 4)."""
        return self._status_pass(L.lib().c2b_problem_triangulate_points, (float(np.deg2rad(float(min_angle_deg))),),
                                 self.num_points(), L.TRI_STATUS, return_status)

    def refine_points(self, rounds=10, lam=1e-4, function_tol=0.0, gradient_tol=0.0, parameter_tol=0.0, return_status=False):
        """Per-point Levenberg-Marquardt on the device (c2b_problem_refine_points): every point is re-minimised
        by itself against the cameras as they are, with its own damping (from `lam`) and its own acceptance, for up to
        `rounds` rounds -- structure-only refinement in one launch.  A point's cost is sum rho(|r|^2) over its observations
        under the handle's loss plus its point prior's; it stops when a tolerance is met (0 disables a test; they are
        levenberg_marquardt_device's, per point).  A point is written only when its cost fell; constant points, points
        with neither an observation nor a prior and points whose start cost is not finite keep their bits.  Masks, priors,
        loss, preconditioner and a checkpoint stay.  Returns dict(converged, max_rounds, unobserved, failed, constant,
        moved): the number of points of each status and of points written; with return_status also the uint8 status per
        point (the dict's order: 0 .. 4)."""
        opt = L.RefineOptions(int(rounds), 0, float(lam), float(function_tol), float(gradient_tol), float(parameter_tol))
        return self._status_pass(L.lib().c2b_problem_refine_points, (C.cast(C.pointer(opt), C.c_void_p),), self.num_points(),
                                 L.REFINE_COUNTS, return_status)

    def set_inner_iterations(self, n):
        """Inner iterations of the LM loops (c2b_problem_set_inner_iterations): with n > 0 solve.levenberg_marquardt and
        levenberg_marquardt_device run refine_points(rounds=n) after every step they apply, before they take the step's cost.
        0 = off, the default.  The setting is the handle's, like the loss: it stays until it is set again (the loops'
        inner_iterations= argument sets it when given and leaves it alone when None)."""
        L.check(L.lib().c2b_problem_set_inner_iterations(self._h, int(n)))

    def inner_iterations(self):
        """the inner iterations in force (set_inner_iterations)"""
        n = C.c_int()
        L.check(L.lib().c2b_problem_get_inner_iterations(self._h, C.byref(n)))
        return n.value

    def triangulate_points_robust(self, max_error, min_angle_deg=1.0, min_inliers=3, max_hypotheses=64, drop_outliers=False,
                                  return_status=False, return_inliers=False):
        """Consensus triangulation on the device (c2b_problem_triangulate_consensus): triangulate_points for a
        list that holds wrong matches.  Per point, candidates are formed from pairs of its rays (at most max_hypotheses <= 64,
        wide pairs first, from the usable observations among the row's first 64), each is scored by how many observations of
        the point it reprojects within max_error in front of their cameras (filter_observations' predicate with in_front),
        and the point is set to the midpoint of the best candidate's inliers -- if there are min_inliers (>= 2) of them,
        they pass the parallax test and none of their cameras sees the point from behind; otherwise it keeps its bits.
        With drop_outliers the observations of the triangulated points that are not inliers are then removed from the
        list as filter_observations removes its own.  Returns dict(triangulated, too_few, degenerate, behind, constant,
        no_consensus, outliers, removed): the number of points of each outcome, the zeros of the inlier mask and how many
        observations left the list; with return_status also (status [n_pts] uint8 in the dict's order 0 .. 5, hyp
        [n_pts] int32 = the selected pair or -1), with return_inliers also the mask [n_obs] uint8 over the list as it was
        at the call."""
        n_pts, n_obs = self.num_points(), self.num_observations()
        counts = np.zeros(6, dtype=np.int64)
        status = np.zeros(n_pts, dtype=np.uint8)
        hyp = np.zeros(n_pts, dtype=np.int32)
        inlier = np.ones(n_obs, dtype=np.uint8)
        removed = C.c_int64()
        L.check(L.lib().c2b_problem_triangulate_consensus(
            self._h, float(np.deg2rad(float(min_angle_deg))), float(max_error), int(min_inliers), int(max_hypotheses),
            L.TRI_DROP_OUTLIERS if drop_outliers else 0, status.ctypes.data_as(C.c_void_p), hyp.ctypes.data_as(C.c_void_p),
            inlier.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), C.byref(removed)))
        if removed.value:
            self._refresh_graph()
        out = dict(zip(L.TRI_CONSENSUS_STATUS, (int(v) for v in counts)))
        out["outliers"] = int(n_obs - np.count_nonzero(inlier))
        out["removed"] = int(removed.value)
        ret = (out,)
        if return_status:
            ret += (status, hyp)
        if return_inliers:
            ret += (inlier,)
        return ret if len(ret) > 1 else out

    def resect_cameras(self, min_points=6, min_gap=1e-4, return_status=False):
        """Camera resection on the device (c2b_problem_resect_cameras): every camera's pose is set from the
        points as they are and its observations -- the minimiser of the object-space error, from a linear start, with f,
        k1 and k2 kept: a start for a solve, not a refinement, and the dual of triangulate_points.  A camera keeps its
        bits when its pose is (partly) constant, when it has fewer than min_points (>= 6) usable observations, when its
        points are too close to coplanar or too little spread (lambda_2 < min_gap lambda_9 of the 9x9 form, or noise
        that swamps the gap), or when a point would lie behind it.  The loss on the handle is ignored; masks, loss,
        preconditioner and a checkpoint stay; the problem is in bal mode afterwards, as after apply_step.  Returns
        dict(resected, too_few, degenerate, behind, constant), the number of cameras of each outcome, and with
        return_status also the uint8 status per camera (the dict's order: 0 .. 4)."""
        return self._status_pass(L.lib().c2b_problem_resect_cameras, (int(min_points), float(min_gap)), self.num_cameras(),
                                 L.RES_STATUS, return_status)

    def refine_cameras(self, rounds=10, lam=1e-4, function_tol=0.0, gradient_tol=0.0, parameter_tol=0.0, return_status=False):
        """Per-camera Levenberg-Marquardt on the device (c2b_problem_refine_cameras): every camera's nine
        parameters are re-minimised against the points as they are, with its own damping (from `lam`) and its own
        acceptance, for up to `rounds` rounds -- motion-only bundle adjustment in one launch, the dual of refine_points and
        the follow-up to resect_cameras.  A camera's cost is sum rho(|r|^2) over its observations under the handle's loss
        plus its centre and intrinsics priors'; parameters constant under set_constant keep their bits; it stops when a
        tolerance is met (0 disables a test).  A camera is written only when its cost fell; cameras with all nine
        parameters constant, cameras with neither an observation nor a prior and cameras whose start cost is not finite
        keep their bits.  Masks, priors, loss, preconditioner and a checkpoint stay; the problem is in bal mode afterwards,
        as after apply_step.  Returns dict(converged, max_rounds, unobserved, failed, constant, moved): the number of
        cameras of each status and of cameras written; with return_status also the uint8 status per camera (the dict's
        order: 0 .. 4)."""
        opt = L.RefineOptions(int(rounds), 0, float(lam), float(function_tol), float(gradient_tol), float(parameter_tol))
        return self._status_pass(L.lib().c2b_problem_refine_cameras, (C.cast(C.pointer(opt), C.c_void_p),), self.num_cameras(),
                                 L.REFINE_COUNTS, return_status)

    def resect_cameras_robust(self, max_error, min_inliers=6, min_gap=1e-4, max_hypotheses=64, drop_outliers=False,
                              return_status=False, return_inliers=False):
        """Consensus resection on the device (c2b_problem_resect_consensus): resect_cameras for a list that
        holds wrong matches.  Per camera, candidate poses are formed from triples of its observations (at most
        max_hypotheses <= 64, widely spaced triples first, from the usable observations among the row's first 64; every
        three-point solution of a triple is a candidate), each is scored by how many observations of the camera it
        reprojects within max_error with the point in front (filter_observations' predicate with in_front), and the
        camera is set to resect_cameras' fit over the best candidate's inliers -- if there are min_inliers (>= 6) of them
        and that fit passes its own tests (min_gap, cheirality); otherwise it keeps its bits.  With drop_outliers the
        observations of the resected cameras that are not inliers are then removed from the list as filter_observations
        removes its own.  Returns dict(resected, too_few, degenerate, behind, constant, no_consensus, outliers, removed):
        the number of cameras of each outcome, the zeros of the inlier mask and how many observations left the list; with
        return_status also (status [n_cam] uint8 in the dict's order 0 .. 5, hyp [n_cam] int32 = the selected triple or
        -1, n_inl [n_cam] int32 = its inlier count), with return_inliers also the mask [n_obs] uint8 over the list as it
        was at the call.  The problem is in bal mode afterwards, as after resect_cameras."""
        n_cam, n_obs = self.num_cameras(), self.num_observations()
        counts = np.zeros(6, dtype=np.int64)
        status = np.zeros(n_cam, dtype=np.uint8)
        hyp = np.zeros(n_cam, dtype=np.int32)
        n_inl = np.zeros(n_cam, dtype=np.int32)
        inlier = np.ones(n_obs, dtype=np.uint8)
        removed = C.c_int64()
        L.check(L.lib().c2b_problem_resect_consensus(
            self._h, float(max_error), int(min_inliers), float(min_gap), int(max_hypotheses), L.RES_DROP_OUTLIERS if drop_outliers else 0,
            status.ctypes.data_as(C.c_void_p), hyp.ctypes.data_as(C.c_void_p), n_inl.ctypes.data_as(C.c_void_p),
            inlier.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), C.byref(removed)))
        if removed.value:
            self._refresh_graph()
        out = dict(zip(L.RES_CONSENSUS_STATUS, (int(v) for v in counts)))
        out["outliers"] = int(n_obs - np.count_nonzero(inlier))
        out["removed"] = int(removed.value)
        ret = (out,)
        if return_status:
            ret += (status, hyp, n_inl)
        if return_inliers:
            ret += (inlier,)
        return ret if len(ret) > 1 else out

    def subset(self, ci, pi, carry=False):
        """BAProblem::subset (src/baproblem.rs:394-423) on the device (c2b_problem_subset): cameras ci and points pi in the
        given order, repeats allowed (a repeated point appears twice and its observations name its last slot);
        observations of dropped points disappear.  Only the two index lists cross PCIe.  Returns a NEW device problem in
        this problem's camera mode, holding this problem's bits: cameras(), points(), row_ptr, pt_idx and observations()
        are the same arrays in either mode.  carry=False: the child's handle state is a new problem's.  carry=True: it
        takes this problem's options, loss, preconditioner, inner iterations, and its constant masks and priors gathered
        by the lists; when neither list repeats an index it also records an origin() and can write_back()."""
        ci = np.asarray(ci, dtype=np.int64).reshape(-1)
        pi = np.asarray(pi, dtype=np.int64).reshape(-1)
        n_cam, n_pts = self.num_cameras(), self.num_points()
        if (len(ci) and (ci.min() < 0 or ci.max() >= n_cam)) or (len(pi) and (pi.min() < 0 or pi.max() >= n_pts)):
            raise L.City2baError(L.ERR_INDEX_OUT_OF_RANGE, "subset: index out of range")
        c32, p32 = np.ascontiguousarray(ci, dtype=np.uint32), np.ascontiguousarray(pi, dtype=np.uint32)
        child = BAProblem(self._device)
        try:
            L.check(L.lib().c2b_problem_subset(self._h, _ptr(c32) if len(c32) else None, len(c32), _ptr(p32) if len(p32) else None,
                                               len(p32), L.SUBSET_CARRY if carry else 0, child._h))
        except Exception:
            child.close()
            raise
        return child._refresh_graph()

    def window(self, cameras, halo=True):
        """A window of this problem as a problem of its own (c2b_problem_window): the seed cameras (`cameras`: an index
        list or a bool mask [n_cam]), the points P they see, and the rim held constant -- with halo, every other camera
        that sees a point of P, all nine parameters constant, with its observations of P; without, no further camera, and
        the points of P seen from outside the window constant.  Every residual that depends on a free variable is in the
        child, so a solve of the child is block-coordinate descent on this problem's cost.  The child carries this
        problem's handle state (masks OR the roles, priors, loss, preconditioner, inner iterations, options) and an
        origin(); write_back() puts its free entities back."""
        n_cam = self.num_cameras()
        a = np.asarray(cameras)
        if a.dtype == np.bool_:
            if a.shape != (n_cam,):
                raise ValueError("window: a bool mask must have shape (%d,)" % n_cam)
            seed = np.ascontiguousarray(a, dtype=np.uint8)
        else:
            idx = np.asarray(a, dtype=np.int64).reshape(-1)
            if len(idx) and (idx.min() < 0 or idx.max() >= n_cam):
                raise L.City2baError(L.ERR_INDEX_OUT_OF_RANGE, "window: camera index out of range")
            seed = np.zeros(n_cam, dtype=np.uint8)
            seed[idx] = 1
        child = BAProblem(self._device)
        try:
            L.check(L.lib().c2b_problem_window(self._h, _ptr(seed), L.WINDOW_HALO if halo else 0, child._h))
        except Exception:
            child.close()
            raise
        return child._refresh_graph()

    def covisibility(self, min_shared=1):
        """The camera covisibility graph of the observation list, built on the device (c2b_problem_covisibility):
        (nbr_ptr [n_cam + 1] uint64, nbr [n_edges] uint32, shared [n_edges] uint32) as numpy arrays -- per camera the cameras
        that observe at least min_shared distinct points it observes too, in ascending index, and how many.  Symmetric, no
        self edge; n_edges counts both directions.  The graph stays in the handle until the list changes or another
        min_shared is asked for, so neighbourhood() at the same threshold does not rebuild it."""
        n = C.c_int64()
        L.check(L.lib().c2b_problem_covisibility(self._h, int(min_shared), C.byref(n)))
        nbr_ptr = np.zeros(self.num_cameras() + 1, dtype=np.uint64)
        nbr, shared = np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
        L.check(L.lib().c2b_problem_get_covisibility(self._h, _ptr(nbr_ptr), _ptr(nbr) if n.value else None, _ptr(shared) if n.value else None,
                                                     None, None))
        return nbr_ptr, nbr, shared

    def covisibility_heavy_cameras(self):
        """how many cameras of the graph the handle holds took the heavy path (more candidate neighbours than a wave's LDS
        table has slots), or None without a graph"""
        n = C.c_int64()
        if L.lib().c2b_problem_get_covisibility(self._h, None, None, None, None, C.byref(n)):
            return None
        return n.value

    def neighbourhood(self, cameras, hops=1, min_shared=1, max_cameras=None, within=None, return_levels=False):
        """This camera and the cameras that see what it sees (c2b_problem_neighbourhood): a breadth-first search over the
        covisibility graph at min_shared from `cameras` (an index list or a bool mask [n_cam]), at most `hops` levels beyond
        them (0: the seeds themselves; None: until nothing new is reached, the seeds' connected components at that
        threshold), inside `within` (an index list or a bool mask, default all cameras; the seeds must lie in it).  With
        max_cameras whole levels are taken while they fit and the first level that does not is cut by (shared points with
        the levels already taken, descending; index, ascending).  Returns the member cameras in ascending index; with
        return_levels also their levels (int32, 0 for a seed)."""
        n_cam = self.num_cameras()

        def mask(a, what):
            a = np.asarray(a)
            if a.dtype == np.bool_:
                if a.shape != (n_cam,):
                    raise ValueError("neighbourhood: a bool mask must have shape (%d,)" % n_cam)
                return np.ascontiguousarray(a, dtype=np.uint8)
            idx = np.asarray(a, dtype=np.int64).reshape(-1)
            if len(idx) and (idx.min() < 0 or idx.max() >= n_cam):
                raise L.City2baError(L.ERR_INDEX_OUT_OF_RANGE, "neighbourhood: %s index out of range" % what)
            m = np.zeros(n_cam, dtype=np.uint8)
            m[idx] = 1
            return m

        seed = mask(cameras, "camera")
        inside = None if within is None else mask(within, "within")
        member, level, n = np.zeros(n_cam, dtype=np.uint8), np.zeros(n_cam, dtype=np.int32), C.c_int64()
        L.check(L.lib().c2b_problem_neighbourhood(self._h, _ptr(seed), -1 if hops is None else int(hops), int(min_shared),
                                                  0 if max_cameras is None else int(max_cameras), None if inside is None else _ptr(inside),
                                                  _ptr(member), _ptr(level), C.byref(n)))
        idx = np.flatnonzero(member)
        return (idx, level[idx]) if return_levels else idx

    def origin(self):
        """where a child of subset(carry=True) / window came from (c2b_problem_get_origin): dict(cam_of [n_cam], pt_of
        [n_pts]: the parent's index of every camera / point; cam_role: 0 seed, 1 halo; pt_role: 1 = shared), or None"""
        n_cam, n_pts, _ = self._sizes()
        out = dict(cam_of=np.zeros(n_cam, dtype=np.uint32), pt_of=np.zeros(n_pts, dtype=np.uint32),
                   cam_role=np.zeros(n_cam, dtype=np.uint8), pt_role=np.zeros(n_pts, dtype=np.uint8))
        if L.lib().c2b_problem_get_origin(self._h, _ptr(out["cam_of"]), _ptr(out["pt_of"]), _ptr(out["cam_role"]), _ptr(out["pt_role"])):
            return None
        return out

    def write_back(self, parent):
        """This child's cameras and points over the parent's (c2b_problem_write_back), component by component where this
        child's masks leave them free now; everything else of the parent keeps its bits.  Both are in bal mode afterwards,
        as after apply_step.  Refused when this problem has no origin, when `parent` is not the problem it was taken from,
        or when the parent's entities were replaced or renumbered since.  Returns dict(cameras, points): cameras with at
        least one free parameter, and free points."""
        a, b = C.c_int64(), C.c_int64()
        L.check(L.lib().c2b_problem_write_back(self._h, parent._h, C.byref(a), C.byref(b)))
        return dict(cameras=a.value, points=b.value)

    # ---- against ground truth: similarity alignment ---------------------------------
    def align(self, ref, on="cameras", scale=True, use_cameras=None, use_points=None, max_dist=None, rounds=5, return_errors=False,
              return_inliers=False):
        """c2b_problem_align: the similarity (s, R, t) that takes this problem onto `ref` (same counts, index i of one corresponds to
        index i of the other) in the least-squares sense, Umeyama's closed form over the camera centres, the points or both
        (`on`), and the errors that remain.  use_cameras / use_points: byte masks, None = all on.  max_dist: after a fit only the
        correspondences within it stay on and the fit is repeated, until the set repeats or after `rounds` re-fits -- trimming from
        the least-squares start, not a consensus search: gross outliers can empty the set, which is reported (status "too_few").
        Neither problem is modified.  Returns dict(status, scale, rotation [3, 3], translation [3], rounds, cameras=dict(n, rmse, mean,
        max, argmax, rot_rmse_deg, rot_mean_deg, rot_max_deg, rot_argmax), points=dict(n, rmse, mean, max, argmax)); with return_errors
        also camera_errors, camera_rotation_errors (radians), point_errors (every entity, masked off or not); with return_inliers
        camera_inliers, point_inliers.  A first fit that fails ("too_few", "degenerate") returns the identity and empty summaries."""
        if on not in L.ALIGN_ON:
            raise ValueError("on must be 'cameras', 'points' or 'both', not %r" % (on,))
        nc, np_, _ = self._sizes()
        o = L.AlignOptions()
        L.lib().c2b_align_options_init(C.byref(o))
        o.on, o.scale, o.rounds = L.ALIGN_ON[on], int(bool(scale)), int(rounds) if max_dist is not None else 0
        o.max_dist = float(max_dist) if max_dist is not None else 0.0
        masks = []
        for name, m, n in (("use_cam", use_cameras, nc), ("use_pt", use_points, np_)):
            if m is not None:
                m = np.ascontiguousarray(np.asarray(m) != 0, dtype=np.uint8)
                if m.shape != (n,):
                    raise L.City2baError(L.ERR_INVALID_ARGUMENT, "align: a mask must have one entry per entity")
                masks.append(m)
                setattr(o, name, m.ctypes.data)
        T, S = L.Similarity(), L.AlignSummary()
        ce, re_, pe = (np.zeros(n) if return_errors else None for n in (nc, nc, np_))
        ci, pi = (np.zeros(n, dtype=np.uint8) if return_inliers else None for n in (nc, np_))
        L.check(L.lib().c2b_problem_align(self._h, ref._h, C.byref(o), C.byref(T), C.byref(S), _ptr(ce), _ptr(re_), _ptr(pe), _ptr(ci), _ptr(pi)))

        def stat(s, scale_=1.0):
            n = s.n
            return dict(n=n, rmse=scale_ * float(np.sqrt(s.sum_sq / n)) if n else 0.0, mean=scale_ * s.sum / n if n else 0.0,
                        max=scale_ * s.max if n else 0.0, argmax=s.argmax)
        cams, rot = stat(S.cameras), stat(S.camera_rotations, 180.0 / np.pi)
        cams.update(rot_rmse_deg=rot["rmse"], rot_mean_deg=rot["mean"], rot_max_deg=rot["max"], rot_argmax=rot["argmax"])
        out = dict(status=L.ALIGN_STATUS[S.status], scale=T.scale, rotation=np.array(T.rotation[:]).reshape(3, 3),
                   translation=np.array(T.translation[:]), rounds=S.rounds, cameras=cams, points=stat(S.points))
        if return_errors:
            out.update(camera_errors=ce, camera_rotation_errors=re_, point_errors=pe)
        if return_inliers:
            out.update(camera_inliers=ci, point_inliers=pi)
        return out

    def transform(self, scale, rotation, translation):
        """c2b_problem_transform: the whole problem moved by a similarity, in place: every point X <- s R X + t, every camera the
        rotation R_c R^T and the centre s R c + t; intrinsics stay, and so does every projection.  The problem is in state mode
        afterwards; rows, transpose, solve buffers, covisibility graph, masks, loss and a checkpoint stay.  Priors hold positions
        in the OLD frame and are left as they are: set them again after a transform.  Refused: a non-finite entry, scale <= 0, a
        rotation that is not orthonormal to 1e-9 or has det < 0."""
        T = L.similarity(scale, rotation, translation)
        L.check(L.lib().c2b_problem_transform(self._h, C.byref(T)))
        return self

    def _refresh_graph(self):
        """host mirrors of the graph (row_ptr, pt_idx) after a device-side change"""
        n_cam, _, n_obs = self._sizes()
        row_ptr = np.zeros(n_cam + 1, dtype=np.uint64)
        pt_idx = np.zeros(n_obs, dtype=np.uint64)
        L.check(L.lib().c2b_problem_download_graph(self._h, _ptr(row_ptr), _ptr(pt_idx)))
        self._row_ptr, self._pt_idx = row_ptr, pt_idx
        return self

    def adopt_visibility(self, mirror=True):
        """BAProblem::from_visibility (src/baproblem.rs:360-376) on the device: the pending result of
        visibility_pairs_compact(fetch=False) / visibility_graph(fetch=False) becomes this problem's vis_graph.
        mirror = False leaves the host copies of the graph (row_ptr(), pt_idx()) stale: for callers that stay on the
        device (export_device) and do not want 12 bytes per observation to cross PCIe"""
        L.check(L.lib().c2b_problem_adopt_visibility(self._h))
        return self._refresh_graph() if mirror else self

    def export_device(self, cam_lo=0, cam_hi=None):
        """c2b_problem_export_device: the resident problem -- or the shard of the camera range [cam_lo, cam_hi) -- as
        torch tensors on the problem's device, copied device to device (Level 1 -> Level 0 without PCIe):
        dict(cam15 [nc,15], pts4 [n_pts,4], row_ptr int64 [nc+1] rebased to 0, pt_idx int32 [n], uv [n,2], obs_lo, n_obs)."""
        import torch
        n_cam, n_pts, _ = self._sizes()
        cam_hi = n_cam if cam_hi is None else int(cam_hi)
        lo, n = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().c2b_problem_export_device(self._h, int(cam_lo), cam_hi, None, None, None, None, None, C.byref(lo), C.byref(n)))
        dev = torch.device("cuda", self._device)
        nc = cam_hi - int(cam_lo)
        out = dict(cam15=torch.empty((nc, 15), dtype=torch.float64, device=dev),
                   pts4=torch.empty((n_pts, 4), dtype=torch.float64, device=dev),
                   row_ptr=torch.empty(nc + 1, dtype=torch.int64, device=dev),
                   pt_idx=torch.empty(n.value, dtype=torch.int32, device=dev),
                   uv=torch.empty((n.value, 2), dtype=torch.float64, device=dev))
        torch.cuda.synchronize(dev)                          # the buffers exist before the problem's own stream writes them
        p = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
        L.check(L.lib().c2b_problem_export_device(self._h, int(cam_lo), cam_hi, p(out["cam15"]), p(out["pts4"]), C.c_void_p(out["row_ptr"].data_ptr()),
                                                  p(out["pt_idx"]), p(out["uv"]), C.byref(lo), C.byref(n)))
        out["obs_lo"], out["n_obs"] = int(lo.value), int(n.value)
        return out

    def cull_host(self, faithful=True):
        """the same through the host implementation (c2b_cull on downloaded arrays); returns a NEW device problem"""
        cams = self.cameras()
        pts = self.points()
        uv = self.observations()
        row_ptr = self._row_ptr.copy()
        pt_idx = self._pt_idx.copy()
        cams, pts, row_ptr, pt_idx, uv = cull_arrays(cams, pts, row_ptr, pt_idx, uv, faithful)
        return BAProblem.from_visibility(cams, pts, row_ptr, pt_idx, uv, self._device)

    @classmethod
    def from_file(cls, path, device=0, fmt=None):
        """BAProblem::from_file (src/baproblem.rs:697-706) straight into the resident problem (c2b_problem_read): a .bbal is
        streamed to the device and decoded there (byte order, index / uv split, range checks, from_vec); .bal text is
        tokenised and parsed on the device too (every number correctly rounded), except files smaller than the option
        text_device_min_bytes (default 64 KiB), files the device parser declines (NaN, more than 19 digits, glued
        numbers) and everything under the option host_text, which go through the host parser and an upload -- the same
        resident state either way.  fmt None = by extension, "text", "binary"."""
        self = cls(device)
        L.check(L.lib().c2b_problem_read(self._h, str(path).encode(), _FORMATS[fmt]))
        return self._refresh_graph()

    @classmethod
    def from_file_text(cls, path, device=0):        # src/baproblem.rs:580-630
        return cls.from_file(path, device, "text")

    @classmethod
    def from_file_binary(cls, path, device=0):      # src/baproblem.rs:632-695
        return cls.from_file(path, device, "binary")

    def write(self, path, fmt=None):
        """BAProblem::write (src/baproblem.rs:768-785) straight from the resident problem: a .bbal image is assembled on
        the device (to_vec, counts, byte order) and only its bytes cross PCIe; so is .bal text (shortest round-trip
        decimals formatted on the device); the option host_text selects the host formatter over a download: same bytes"""
        L.check(L.lib().c2b_problem_write(self._h, str(path).encode(), _FORMATS[fmt]))

    def write_text(self, path):                     # src/baproblem.rs:709-733
        self.write(path, "text")

    def write_binary(self, path):                   # src/baproblem.rs:736-764
        self.write(path, "binary")

    def visibility_pairs(self, cam_idx, pt_idx, max_dist):
        """predicate of the generator loops (src/synthetic.rs:285-291; src/generate.rs:448-454)"""
        cam_idx = np.ascontiguousarray(cam_idx, dtype=np.uint32)
        pt_idx = np.ascontiguousarray(pt_idx, dtype=np.uint32)
        n = len(cam_idx)
        if len(pt_idx) != n:
            raise L.City2baError(L.ERR_INVALID_ARGUMENT, "cam_idx and pt_idx differ in length")
        uv = np.empty((n, 2))
        keep = np.empty(n, dtype=np.uint8)
        L.check(L.lib().c2b_problem_visibility_pairs(self._h, n, _ptr(cam_idx), _ptr(pt_idx), float(max_dist),
                                                     _ptr(uv), _ptr(keep)))
        return uv, keep

    def visibility_within_distance(self, max_dist, occlusion=False, block_length=20.0, block_inset=1.0, fetch=True):
        """the synthetic generators' whole visibility loop on the device (src/synthetic.rs:268-297, :353-378): candidates
        within max_dist of each camera centre (a cell list in place of rstar's locate_within_distance), hits_building when
        `occlusion`, the predicate, kept lists per camera in ascending point index.  Returns (row_ptr, pt_idx, uv), or
        the row pointer only with fetch=False (the lists stay on the device for adopt_visibility)."""
        row_ptr = np.zeros(self.num_cameras() + 1, dtype=np.uint64)
        L.check(L.lib().c2b_problem_visibility_within_distance(self._h, float(max_dist), int(bool(occlusion)), float(block_length),
                                                               float(block_inset), _ptr(row_ptr)))
        if not fetch:
            return row_ptr
        n = int(row_ptr[-1])
        kept = np.empty(n, dtype=np.uint64)
        uv = np.empty((n, 2))
        L.check(L.lib().c2b_problem_visibility_dense_fetch(self._h, _ptr(kept), _ptr(uv)))
        return row_ptr, kept, uv

    def visibility_pairs_compact(self, cam_idx, pt_idx, max_dist, fetch=True):
        """the same predicate with the kept pairs compacted on the device (cam_idx non-decreasing): returns the CSR
        graph (row_ptr u64, pt_idx u64, uv) of the survivors in candidate order; fetch=False leaves the lists on the
        device (for adopt_visibility) and returns the row pointer only"""
        cam_idx = np.ascontiguousarray(cam_idx, dtype=np.uint32)
        pt_idx = np.ascontiguousarray(pt_idx, dtype=np.uint32)
        if len(pt_idx) != len(cam_idx):
            raise L.City2baError(L.ERR_INVALID_ARGUMENT, "cam_idx and pt_idx differ in length")
        row_ptr = np.zeros(self.num_cameras() + 1, dtype=np.uint64)
        L.check(L.lib().c2b_problem_visibility_pairs_compact(self._h, len(cam_idx), _ptr(cam_idx), _ptr(pt_idx),
                                                             float(max_dist), _ptr(row_ptr)))
        if not fetch:
            return row_ptr
        n = int(row_ptr[-1])
        kept = np.empty(n, dtype=np.uint64)
        uv = np.empty((n, 2))
        L.check(L.lib().c2b_problem_visibility_dense_fetch(self._h, _ptr(kept), _ptr(uv)))
        return row_ptr, kept, uv


class _PinnedBlock:
    """owner of one c2b_host_alloc block; arrays made from it keep it alive through their .base chain"""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        L.check(L.lib().c2b_host_alloc(C.byref(self.ptr), self.nbytes))
        self.__array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr.value or 0, False), "version": 3}

    def __del__(self):
        try:
            if self.ptr:
                L.lib().c2b_host_free(self.ptr)
                self.ptr = C.c_void_p()
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float64):
    """np.empty in page-locked host memory (c2b_host_alloc): the destination that takes device results at link speed"""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    if n == 0:
        return np.empty(shape, dtype=dtype)
    return np.asarray(_PinnedBlock(n)).view(dtype).reshape(shape)


# ---- host-array helpers over the C ABI (no GPU involved) ------------------------------------------------
def cull_arrays(cams, pts, row_ptr, pt_idx, uv, faithful=True, step="cull"):
    """c2b_cull on numpy arrays; cams is [n, stride] (cam15 or bal9 rows).  Returns the culled copies.
    step = "cull" | "lcc" (largest_connected_component once) | "singletons" (remove_singletons once)"""
    cams = np.array(cams, dtype=np.float64, order="C", copy=True)
    cams = cams.reshape(len(cams), -1) if cams.size else cams.reshape(0, cams.shape[-1] if cams.ndim == 2 else 15)
    pts = np.array(pts, dtype=np.float64, order="C", copy=True).reshape(-1, 3)
    row_ptr = np.array(row_ptr, dtype=np.uint64, order="C", copy=True)
    pt_idx = np.array(pt_idx, dtype=np.uint64, order="C", copy=True)
    uv = np.array(uv, dtype=np.float64, order="C", copy=True).reshape(-1, 2)
    if len(row_ptr) != len(cams) + 1:
        raise L.City2baError(L.ERR_INVALID_ARGUMENT, "row_ptr must have n_cameras + 1 entries")
    stride = cams.shape[1] if cams.ndim == 2 and len(cams) else 0
    nc, npts = C.c_int64(len(cams)), C.c_int64(len(pts))
    args = (C.byref(nc), _ptr(cams), int(stride), C.byref(npts), _ptr(pts), _ptr(row_ptr), _ptr(pt_idx), _ptr(uv))
    if step == "cull":
        L.check(L.lib().c2b_cull(*args, int(bool(faithful))))
    elif step == "lcc":
        L.check(L.lib().c2b_largest_connected_component(*args, int(bool(faithful))))
    elif step == "singletons":
        L.check(L.lib().c2b_remove_singletons(*args))
    else:
        raise L.City2baError(L.ERR_INVALID_ARGUMENT, "step must be 'cull', 'lcc' or 'singletons'")
    n_obs = int(row_ptr[nc.value])
    return (cams[:nc.value].copy(), pts[:npts.value].copy(), row_ptr[:nc.value + 1].copy(), pt_idx[:n_obs].copy(),
            uv[:n_obs].copy())


_FORMATS = {None: -1, "text": 0, "binary": 1}


def read_bal(path, fmt=None):
    """(bal9 [n,9], pts [m,3], row_ptr, pt_idx, uv) from a .bal / .bbal file; fmt None = by extension (from_file),
    "text" = from_file_text, "binary" = from_file_binary (src/baproblem.rs:580, :632, :697)."""
    h = C.c_void_p()
    L.check(L.lib().c2b_bal_read_as(str(path).encode(), _FORMATS[fmt], C.byref(h)))
    try:
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib().c2b_bal_sizes(h, C.byref(a), C.byref(b), C.byref(c)))
        bal9, pts = np.empty((a.value, 9)), np.empty((b.value, 3))
        row_ptr = np.empty(a.value + 1, dtype=np.uint64)
        pt_idx = np.empty(c.value, dtype=np.uint64)
        uv = np.empty((c.value, 2))
        L.check(L.lib().c2b_bal_copy(h, _ptr(bal9), _ptr(pts), _ptr(row_ptr), _ptr(pt_idx), _ptr(uv)))
    finally:
        L.lib().c2b_bal_close(h)
    return bal9, pts, row_ptr, pt_idx, uv


def format_f64(values):
    """the texts write_text gives these doubles (Rust's `{}`: shortest round-trip digits, no exponent) -- c2b_format_f64"""
    v = np.ascontiguousarray(values, dtype=np.float64).ravel()
    buf = C.create_string_buffer(max(1, 331 * len(v)))
    n = C.c_int64()
    L.check(L.lib().c2b_format_f64(len(v), _ptr(v), buf, len(buf), C.byref(n)))
    return buf.raw[:n.value].decode("ascii").split("\n")[:-1]


def parse_f64(tokens):
    """(values, status) of decimal tokens as from_file_text reads them -- c2b_parse_f64: status 0 parsed (correctly
    rounded), 1 a spelling left to strtod, 2 too many digits / an undecided rounding"""
    text = " ".join(tokens).encode("ascii")
    vals, st = np.empty(len(tokens)), np.empty(len(tokens), dtype=np.int32)
    L.check(L.lib().c2b_parse_f64(text, len(text), len(tokens), _ptr(vals), _ptr(st)))
    return vals, st


def write_bal(path, bal9, pts, row_ptr, pt_idx, uv, fmt=None):
    """write (by extension), write_text or write_binary (src/baproblem.rs:709, :736, :768)"""
    bal9 = _f64(bal9, (-1, 9))
    pts = _f64(pts, (-1, 3))
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
    pt_idx = np.ascontiguousarray(pt_idx, dtype=np.uint64)
    uv = _f64(uv, (-1, 2))
    L.check(L.lib().c2b_bal_write_as(str(path).encode(), _FORMATS[fmt], len(bal9), _ptr(bal9), len(pts), _ptr(pts),
                                     _ptr(row_ptr), _ptr(pt_idx), _ptr(uv)))
