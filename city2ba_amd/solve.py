"""Levenberg-Marquardt on a resident BAProblem: BAProblem.solve_step (the damped Gauss-Newton step by PCG on the
cameras' Schur complement, on the device) and apply_step, with Nielsen's update of the damping; optionally under a
robust loss (BAProblem.set_loss), by iteratively reweighted least squares, with chosen camera parameters and points
held constant (BAProblem.set_constant) and with priors on camera centres, intrinsics and points (BAProblem.set_priors);
and the usual pipeline around it (solve_filtered): a robust solve, the observations whose residual is still large
dropped on the device (BAProblem.filter_observations), a last solve without a loss; and resection-intersection
alternation (alternate): BAProblem.refine_cameras and refine_points in turn."""

LAMBDA_MIN, LAMBDA_MAX = 1e-20, 1e32                # the damping c2b_problem_solve_step accepts (C2B_STEP_LAMBDA_MIN / _MAX)
# bits of a camera's constant mask (BAProblem.set_constant; C2B_CONST_*): parameter k of to_vec order is bit k
ROTATION, TRANSLATION, POSE = 0x007, 0x038, 0x03f
FOCAL, K1, K2, INTRINSICS = 0x040, 0x080, 0x100, 0x1c0
ALL = 0x1ff


def _clamp(lam):
    return min(max(lam, LAMBDA_MIN), LAMBDA_MAX)


def levenberg_marquardt(ba, iterations=10, lam=1e-4, max_iters=100, rel_tol=1e-6, loss=None, loss_scale=1.0, preconditioner=None, constant=None,
                        priors=None, inner_iterations=None, schur=None, linear_solver=None):
    """`iterations` LM iterations on ba in place.  An iteration solves the damped step, applies it and keeps it when the
    sum of squared residuals falls: gain ratio rho = (e0 - e1) / model_decrease, then lam *= max(1/3, 1 - (2 rho - 1)^3)
    and nu = 2 (accepted), or lam *= nu and nu *= 2 (rejected; cameras and points are restored bit for bit); lam is held
    in [LAMBDA_MIN, LAMBDA_MAX] throughout.  Returns the history: one dict per iteration -- error (sum |r|^2 before it),
    lam (the damping it used), accepted, pcg_iterations, status (the solve's) -- and the final sum |r|^2 as the last
    entry's 'error_after'.
    loss = "huber" | "cauchy" | "soft_l1" with loss_scale (BAProblem.set_loss, which this calls: the loss stays on ba): the
    steps are those of iteratively reweighted least squares, the quantity compared before and after a step is
    ba.robust_cost() = sum rho(|r|^2) -- 'error', 'error_after' and the entry 'cost' hold it -- and the gain ratio
    divides by the weighted model decrease the step reports.  loss = None leaves ba's loss as it is: a loss the caller
    set with ba.set_loss is in force all the same (the step is the reweighted one, so the cost must be the robust one);
    with none in force the loop runs as it always did and 'cost' repeats 'error'.
    preconditioner = "block_jacobi" | "schur_jacobi" (BAProblem.set_preconditioner, which this calls: it stays on ba);
    None leaves ba's as it is.  It changes how many PCG iterations a step takes, not what the step converges to.
    constant = (cameras, points) as BAProblem.set_constant takes them (which this calls: the masks stay on ba); None leaves
    ba's masks as they are.  Constant entries get a zero step and keep their bits through accepted and rejected iterations
    (the restore after a rejected step is an upload of the same counts, which keeps the masks).
    priors = dict(...) of BAProblem.set_priors' keywords (which this calls: the priors stay on ba); None leaves ba's priors as
    they are.  With priors in force the steps are those of the stacked system and the quantity compared -- 'error', 'cost',
    'error_after' -- is the observations' cost + ba.prior_cost(), added in that order.
    inner_iterations = n (BAProblem.set_inner_iterations, which this calls: it stays on ba); None leaves ba's setting as it
    is.  With n > 0 in force, after a step is applied and before its cost is taken, every point is re-minimised against the
    moved cameras by ba.refine_points(rounds=n) (Ceres' inner iterations with the points as the inner block).
    The cost compared is the one after the refinement, so the gain ratio may exceed 1; a rejected step restores the points
    as before.
    schur = "implicit" | "explicit" (BAProblem.set_schur, which this calls: it stays on ba); None leaves ba's setting as it is.
    Explicit forms the reduced camera system once per step and iterates on the stored blocks: the steps converge
    to the same solution.
    linear_solver = "pcg" | "cholesky" (BAProblem.set_linear_solver, which this calls: it stays on ba, as schur does); None leaves
    ba's setting as it is.  Under "cholesky" every step is the exact solution of the damped system by a dense factorisation
    (DESIGN 4.23): 'pcg_iterations' is 0 in every entry, and max_iters and rel_tol are checked and not used."""
    if schur is not None:
        ba.set_schur(schur)
    if linear_solver is not None:
        ba.set_linear_solver(linear_solver)
    if inner_iterations is not None:
        ba.set_inner_iterations(inner_iterations)
    n_inner = ba.inner_iterations()
    if priors is not None:
        ba.set_priors(**priors)
    if constant is not None:
        ba.set_constant(*constant)
    if preconditioner is not None:
        ba.set_preconditioner(preconditioner)
    if loss is not None:
        ba.set_loss(loss, loss_scale)
    robust = ba.loss[0] is not None
    ba.apply_step(None, None)                       # bal mode: bal9 is then what the problem holds exactly
    bal9, pts = ba.cameras_bal(), ba.points()
    row_ptr, pt_idx, uv = ba.row_ptr.copy(), ba.pt_idx.copy(), ba.observations()
    nu = 2.0
    lam = _clamp(lam)
    history = []
    with_priors = any(ba.priors["active"])
    cost = lambda: ba.robust_cost() if robust else ba.total_reprojection_error(2.0) ** 2
    if with_priors:
        observed = cost
        cost = lambda: observed() + ba.prior_cost()
    e0 = cost()
    for _ in range(int(iterations)):
        dc, dp, info = ba.solve_step(lam, max_iters=max_iters, rel_tol=rel_tol)
        ba.apply_step(dc, dp)
        if n_inner:
            ba.refine_points(rounds=n_inner)
        e1 = cost()
        md = info["model_decrease"]
        rho = (e0 - e1) / md if md > 0.0 else -1.0
        accepted = rho > 0.0 and e1 < e0
        history.append(dict(error=e0, cost=e0, lam=lam, accepted=accepted, pcg_iterations=info["iterations"], status=info["status"]))
        if accepted:
            lam = _clamp(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            nu = 2.0
            bal9, pts = ba.cameras_bal(), ba.points()
            e0 = e1
        else:
            ba._upload(bal9, True, pts, row_ptr, pt_idx, uv)
            lam = _clamp(lam * nu)
            nu *= 2.0
    if history:
        history[-1]["error_after"] = e0
    return history


def levenberg_marquardt_device(ba, iterations=10, lam=1e-4, max_iters=100, rel_tol=1e-6, function_tol=0.0, gradient_tol=0.0,
                               parameter_tol=0.0, loss=None, loss_scale=1.0, preconditioner=None, constant=None, priors=None,
                               inner_iterations=None, schur=None, linear_solver=None):
    """levenberg_marquardt's loop inside the library (c2b_problem_levenberg_marquardt): the same steps, the same damping
    and the same numbers, with a device-side checkpoint and rollback where the loop above downloads and uploads, and with
    stopping tests.  Returns (history, summary).
    history: one dict per iteration with levenberg_marquardt's keys (error, cost, lam, accepted, pcg_iterations, status;
    'error_after' in the last entry) plus cost_trial (the cost with the step applied; the cost itself when the step was
    not applied), model_decrease, gradient_max = max(|gc|, |gp|) at the state the step was solved at, step_norm =
    |(dc, dp)|, x_norm = |(cameras_bal, points)| and pcg_rel_residual.
    summary: dict(iterations, termination, reason, initial_cost, final_cost, lam_next); termination 0 = `iterations`
    reached, 1 = function tolerance (cost - cost_trial <= function_tol cost after an accepted step, which is kept), 2 =
    gradient tolerance (gradient_max <= gradient_tol; the step is not applied), 3 = parameter tolerance (step_norm <=
    parameter_tol (x_norm + parameter_tol); the step is not applied), 4 = the cost or the gradient is not finite (the state
    is the last accepted one).  A tolerance of 0 disables its test: with all three at 0 this is levenberg_marquardt,
    iteration for iteration.  loss, preconditioner, constant and priors as there: with priors in force every cost is the
    observations' cost + the priors', and the gradient test reads the gradient of the stacked system.
    inner_iterations and schur as there: set on the handle when given, left as they are when None; the library's loop honours
    the handle's.  linear_solver as there too."""
    import ctypes as C

    from . import _lib as L
    if schur is not None:
        ba.set_schur(schur)
    if linear_solver is not None:
        ba.set_linear_solver(linear_solver)
    if priors is not None:
        ba.set_priors(**priors)
    if constant is not None:
        ba.set_constant(*constant)
    if preconditioner is not None:
        ba.set_preconditioner(preconditioner)
    if loss is not None:
        ba.set_loss(loss, loss_scale)
    if inner_iterations is not None:
        ba.set_inner_iterations(inner_iterations)
    n = int(iterations)
    opt = L.LmOptions(n, int(max_iters), float(lam), float(rel_tol), float(function_tol), float(gradient_tol), float(parameter_tol))
    entries = (L.LmIteration * max(n, 1))()
    s = L.LmSummary()
    L.check(L.lib().c2b_problem_levenberg_marquardt(ba._h, C.byref(opt), entries, n, C.byref(s)))
    history = []
    for e in entries[:s.iterations]:
        d = dict(error=e.cost, cost=e.cost, lam=e.lam, accepted=bool(e.accepted), pcg_iterations=e.pcg_iterations, status=e.status)
        d.update({k: getattr(e, k) for k in ("cost_trial", "model_decrease", "gradient_max", "step_norm", "x_norm", "pcg_rel_residual")})
        history.append(d)
    if history:
        history[-1]["error_after"] = s.final_cost
    summary = dict(iterations=s.iterations, termination=s.termination, reason=L.LM_TERMINATIONS[s.termination],
                   initial_cost=s.initial_cost, final_cost=s.final_cost, lam_next=s.lambda_next)
    return history, summary


def alternate(ba, sweeps=10, camera_rounds=5, point_rounds=5, function_tol=0.0, lam=1e-4, loss=None, loss_scale=1.0, constant=None, priors=None):
    """Resection-intersection alternation on ba in place: per sweep ba.refine_cameras(rounds=camera_rounds, lam=lam), then
    ba.refine_points(rounds=point_rounds, lam=lam), then the cost -- full bundle adjustment as block-coordinate descent, two
    launches per sweep, without a Schur complement or a PCG.  Every camera and every point has its own damping
    and acceptance and never ends a call with a higher cost of its own, so the total cost does not rise.  The cost is the one
    the LM loops compare: the observations' (ba.robust_cost() under a loss, else the sum of squared residuals), then, with
    priors in force, + ba.prior_cost().  It stops early after a sweep whose relative decrease, (before - after) / before, is
    <= function_tol (0 disables the test: every sweep is run, as `city2ba refine --alternate N` runs them).  loss, constant and priors as levenberg_marquardt takes them: set on ba when given
    (they stay), left as they are when None.
    The gauge is the caller's business: nothing here fixes the seven degrees of freedom of the whole problem, and alternation
    drifts along them only slowly, but a comparison against ground truth needs them held -- hold cameras with set_constant
    (constant=) or tie them down with set_priors (priors=).
    Returns dict(costs, cameras, points, sweeps): costs = the cost before the first sweep and after every sweep run
    (sweeps + 1 entries), cameras and points = the status dicts of the last sweep's two calls (None when sweeps is 0)."""
    if priors is not None:
        ba.set_priors(**priors)
    if constant is not None:
        ba.set_constant(*constant)
    if loss is not None:
        ba.set_loss(loss, loss_scale)
    robust = ba.loss[0] is not None
    with_priors = any(ba.priors["active"])

    def cost():
        observed = ba.robust_cost() if robust else ba.total_reprojection_error(2.0) ** 2
        return observed + ba.prior_cost() if with_priors else observed

    costs = [cost()]
    cams = pts = None
    for _ in range(int(sweeps)):
        cams = ba.refine_cameras(rounds=camera_rounds, lam=lam)
        pts = ba.refine_points(rounds=point_rounds, lam=lam)
        costs.append(cost())
        if function_tol > 0.0 and costs[-2] - costs[-1] <= function_tol * costs[-2]:
            break
    return dict(costs=costs, cameras=cams, points=pts, sweeps=len(costs) - 1)


def solve_filtered(ba, max_error, rounds=1, in_front=False, **lm):
    """Robust solve, reject outliers, solve again -- all on the resident problem.  `rounds` times
    levenberg_marquardt_device(ba, **lm) followed by ba.filter_observations(max_error, in_front), then a last
    levenberg_marquardt_device with loss="squared", which clears the loss (it stays cleared on ba).  **lm is what
    levenberg_marquardt_device takes (iterations, lam, tolerances, loss, loss_scale, preconditioner, constant,
    inner_iterations); the last
    solve takes the same arguments but for the loss.  Returns (solves, removed): solves = the (history, summary) of every
    solve, rounds + 1 of them, removed = the observations each round's filter dropped.
    A filter can leave cameras or points with too few observations to constrain them (a camera needs more than 3, a point
    more than 1 for cull() to keep them); nothing is culled here, because a cull renumbers the entities and drops the
    masks: ba.cull() is the caller's call."""
    solves, removed = [], []
    for _ in range(int(rounds)):
        solves.append(levenberg_marquardt_device(ba, **lm))
        removed.append(ba.filter_observations(max_error, in_front=in_front))
    last = dict(lm)
    last.pop("loss_scale", None)
    last["loss"] = "squared"
    solves.append(levenberg_marquardt_device(ba, **last))
    return solves, removed


def solve_window(ba, cameras, halo=True, **lm):
    """Local bundle adjustment of one window, on the device: ba.window(cameras, halo), levenberg_marquardt_device(child,
    **lm), child.write_back(ba), child.close().  The rim of the window is held constant and every residual that depends
    on a free variable is in the child, so the child's cost reduction is ba's: one step of block-coordinate descent on
    the full cost.  The child carries ba's masks, priors, loss, preconditioner and inner iterations; **lm is what
    levenberg_marquardt_device takes (a `constant` or `priors` given there would replace what the window installed, the
    rim's masks included, and must be sized for the child).  ba is in bal mode afterwards.  Returns the LM summary plus
    cameras, points, observations (the child's sizes), written = write_back's counts and history = the iterations."""
    child = ba.window(cameras, halo=halo)
    try:
        history, summary = levenberg_marquardt_device(child, **lm)
        out = dict(summary)
        out["cameras"], out["points"], out["observations"] = child._sizes()
        out["written"] = child.write_back(ba)
        out["history"] = history
        return out
    finally:
        child.close()


def solve_neighbourhood(ba, cameras, hops=1, min_shared=1, max_cameras=None, halo=True, **lm):
    """solve_window on a covisibility neighbourhood: the seeds of the window are ba.neighbourhood(cameras, hops, min_shared,
    max_cameras) -- `cameras` and every camera within `hops` edges of the covisibility graph at min_shared, cut to
    max_cameras by shared points -- and the rim is the window's as ever.  Returns solve_window's summary plus seeds (the
    window's cameras, ascending) and levels (their distance from `cameras` in the graph)."""
    seeds, levels = ba.neighbourhood(cameras, hops=hops, min_shared=min_shared, max_cameras=max_cameras, return_levels=True)
    out = solve_window(ba, seeds, halo=halo, **lm)
    out["seeds"], out["levels"] = seeds, levels
    return out


def solve_windows(ba, size, stride=None, sweeps=1, halo=True, by="index", min_shared=1, **lm):
    """solve_window over windows of `size` cameras, over all cameras, `sweeps` times.
    by="index": windows of consecutive camera indices every `stride` (default: size).  Returns the per-window summaries in the
    order solved, each with lo and hi (its cameras lo .. hi - 1) and sweep.
    by="covisibility": windows grown over the covisibility graph at min_shared, for lists whose index order does not follow
    the scene.  Per sweep every camera starts as to-do; until none is left, the lowest to-do index is the seed, the window is
    ba.neighbourhood([seed], hops=None, max_cameras=size, within=the to-do cameras), it is solved and its cameras are done.
    The windows of a sweep partition the cameras.  `stride` is refused.  Each summary carries seed, seeds (the window's
    cameras), levels and sweep."""
    size = int(size)
    if by == "covisibility":
        if stride is not None:
            raise ValueError("solve_windows: stride has no meaning with by='covisibility'")
        if size < 1:
            raise ValueError("solve_windows: size must be at least 1")
        import numpy as np
        n_cam = ba.num_cameras()
        out = []
        for sweep in range(int(sweeps)):
            todo = np.ones(n_cam, dtype=bool)
            first = 0
            while first < n_cam:
                seeds, levels = ba.neighbourhood([first], hops=None, min_shared=min_shared, max_cameras=size, within=todo, return_levels=True)
                s = solve_window(ba, seeds, halo=halo, **lm)
                s.update(seed=first, seeds=seeds, levels=levels, sweep=sweep)
                out.append(s)
                todo[seeds] = False
                while first < n_cam and not todo[first]:
                    first += 1
        return out
    if by != "index":
        raise ValueError("solve_windows: by must be 'index' or 'covisibility', not %r" % (by,))
    stride = size if stride is None else int(stride)
    if size < 1 or stride < 1:
        raise ValueError("solve_windows: size and stride must be at least 1")
    n_cam = ba.num_cameras()
    out = []
    for sweep in range(int(sweeps)):
        for lo in range(0, n_cam, stride):
            hi = min(lo + size, n_cam)
            s = solve_window(ba, range(lo, hi), halo=halo, **lm)
            s.update(lo=lo, hi=hi, sweep=sweep)
            out.append(s)
            if hi == n_cam:
                break
    return out


def compare(ba, ref, **align):
    """How close ba came to the truth `ref` (same counts, corresponding indices): ba.align(ref, **align) -- the best similarity
    between the two frames, which the seven gauge freedoms leave open, and the camera and point errors that remain after it.
    Both problems are left untouched.  The keywords are BAProblem.align's (on, scale, use_cameras, use_points, max_dist, rounds,
    return_errors, return_inliers); returns its dict."""
    return ba.align(ref, **align)
