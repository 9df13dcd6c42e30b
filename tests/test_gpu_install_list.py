"""The one routine that replaces the resident problem's observation list (install_observations, csrc/capi_graph.hpp) held to
what its three callers -- cull, adopt_visibility, filter_observations -- did when each spelt it out: on a handle whose rows,
transpose and solve buffers of the OLD list exist (a solve_step ran), the state after the call is, bit for bit, the state of
a twin uploaded with the downloaded lists; and what each caller owns beside the list is dropped or kept as before: cull drops
the masks and the checkpoint, adopt and the filter keep both.  (tests/test_gpu_filter.py has the filter's twin without them.)"""
import numpy as np
import pytest

import oracle as O
from _problems import dome_problem, grid_cameras_points
from test_gpu_schur_step import _bits, _np, env  # noqa: F401  (env is the module fixture)

pytestmark = pytest.mark.gpu
INTRINSICS = 0x1c0                           # f, k1, k2 in to_vec order


def _use(ba):
    """rows (error sum), transpose (normal equations) and solve buffers of the list the handle holds now"""
    ba.total_reprojection_error(2.0)
    ba.normal_equations()
    ba.solve_step(1e-2)


def _twin(c2b, ba, masks=None):
    """a fresh handle uploaded with what `ba` holds now"""
    twin = c2b.BAProblem.from_bal(ba.cameras_bal(), ba.points(), ba.row_ptr, ba.pt_idx, ba.observations(), device=0)
    if masks is not None:
        twin.set_constant(*masks)
    return twin


def _same_state(ba, twin):
    assert ba.total_reprojection_error(2.0) == twin.total_reprojection_error(2.0)
    a, b = ba.normal_equations(), twin.normal_equations()
    for x, y in zip(a[:4], b[:4]):
        assert _bits(_np(x), _np(y))
    assert a[4] == b[4]
    (dc, dp, info), (dc2, dp2, info2) = ba.solve_step(1e-2), twin.solve_step(1e-2)
    assert _bits(_np(dc), _np(dc2)) and _bits(_np(dp), _np(dp2)) and info == info2, (info, info2)
    return _np(dc)


def _checkpoint_in_force(env, ba, b0, p0):
    """a step away from the checkpointed state, and back"""
    torch, dev = env["torch"], env["dev"]
    rng = np.random.default_rng(5)
    ba.apply_step(torch.from_numpy(rng.normal(scale=1e-4, size=b0.shape)).to(dev), torch.from_numpy(rng.normal(scale=1e-4, size=p0.shape)).to(dev))
    assert not _bits(ba.cameras_bal(), b0) and not _bits(ba.points(), p0)
    ba.rollback()
    assert _bits(ba.cameras_bal(), b0) and _bits(ba.points(), p0)


def cull_case():
    """dome_problem(dup=True) + a second component (3 cameras that see 5 points of their own, all of them) + one point seen
    once, by the camera with the longest row: cull removes entities of both kinds beyond the dome's own"""
    P = dome_problem(dup=True)
    rng = np.random.default_rng(23)
    n_cam, n_pts = len(P["bal9"]), len(P["pts"])
    bal9 = np.concatenate([P["bal9"], P["bal9"][:3] + rng.normal(scale=1e-3, size=(3, 9))])
    pts = np.concatenate([P["pts"], rng.uniform(-2.0, 2.0, size=(6, 3))])
    row_ptr = P["row_ptr"].astype(np.int64)
    rows = [P["pt_idx"][row_ptr[c]:row_ptr[c + 1]].astype(np.int64) for c in range(n_cam)]
    longest = int(np.argmax(np.diff(row_ptr)))
    rows[longest] = np.insert(rows[longest], 7, n_pts + 5)                   # the point seen once
    rows += [np.arange(n_pts, n_pts + 5) for _ in range(3)]                  # the second component
    new_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    pt_idx = np.concatenate(rows).astype(np.uint64)
    uv = O.project_observations(O.camera_from_bal(bal9), pts, new_ptr, pt_idx) + rng.normal(scale=1e-3, size=(len(pt_idx), 2))
    return dict(bal9=bal9, pts=pts, row_ptr=new_ptr, pt_idx=pt_idx, uv=uv)


def test_cull_installs_the_list_and_drops_what_described_the_entities(env):
    import city2ba_amd as c2b
    from city2ba_amd.baproblem import cull_arrays
    P = cull_case()
    n_cam, n_pts = len(P["bal9"]), len(P["pts"])
    hc, hp, hrow, hpi, _ = cull_arrays(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"])       # the host's c2b_cull
    assert 3 < len(hc) <= n_cam - 3 and 1 < len(hp) <= n_pts - 6, (len(hc), len(hp))       # both counts drop, something is left
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    cm = np.zeros(n_cam, dtype=np.uint16)
    cm[1::2] = INTRINSICS
    pm = np.zeros(n_pts, dtype=bool)
    pm[::7] = True
    ba.set_constant(cm, pm)
    ba.checkpoint()
    _use(ba)
    ba.cull()
    print("INSTALL cull: %d -> %d cameras, %d -> %d points, %d -> %d observations"
          % (n_cam, ba.num_cameras(), n_pts, ba.num_points(), len(P["pt_idx"]), ba.num_observations()))
    assert ba.num_cameras() == len(hc) and ba.num_points() == len(hp)
    assert _bits(ba.row_ptr, hrow) and _bits(ba.pt_idx, hpi)
    twin = _twin(c2b, ba)
    assert np.abs(_same_state(ba, twin)).max() > 0.0
    got_c, got_p = ba.constant()
    assert not got_c.any() and not got_p.any()
    with pytest.raises(c2b.City2baError):
        ba.rollback()
    ba.close()
    twin.close()


def test_adopt_visibility_installs_the_list_and_keeps_masks_and_checkpoint(env):
    import city2ba_amd as c2b
    cams, pts = grid_cameras_points(3, cpb=10, ppb=20, L=5.0)              # the small grid of tests/test_gpu_cells.py
    ba = c2b.BAProblem.from_visibility(cams, pts, np.zeros(len(cams) + 1, dtype=np.uint64), [], np.zeros((0, 2)))
    ba.visibility_within_distance(10.0, False, 5.0, 1.0)
    ba.adopt_visibility()
    n_first = ba.num_observations()
    cm = np.zeros(len(cams), dtype=np.uint16)
    cm[::3] = INTRINSICS
    pm = np.zeros(len(pts), dtype=bool)
    pm[::5] = True
    ba.set_constant(cm, pm)
    ba.checkpoint()
    b0, p0 = ba.cameras_bal(), ba.points()
    want_c, want_p = ba.constant()
    _use(ba)                                                               # of the first list
    row, kept, uv = ba.visibility_within_distance(6.0, False, 5.0, 1.0)    # a shorter one, from the checkpointed state
    assert 0 < len(kept) < n_first
    ba.adopt_visibility()
    print("INSTALL adopt: %d -> %d observations" % (n_first, ba.num_observations()))
    assert _bits(ba.row_ptr, row) and _bits(ba.pt_idx, kept) and _bits(ba.observations().reshape(-1, 2), uv.reshape(-1, 2))
    twin = _twin(c2b, ba, (cm, pm))
    _same_state(ba, twin)
    got_c, got_p = ba.constant()
    assert _bits(got_c, want_c) and _bits(got_p, want_p) and want_c.any() and want_p.any()
    _checkpoint_in_force(env, ba, b0, p0)
    ba.close()
    twin.close()


def test_filter_installs_the_list_and_keeps_masks_and_checkpoint(env):
    import city2ba_amd as c2b
    import _filterref as F
    import _solvecheck as SC
    P = F.dome_case(True, False)
    t = P["thresholds"][0]
    _, rows, pi, uv, removed = F.case_reference(P, t)
    ba = c2b.BAProblem.from_bal(P["bal9"], P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], device=0)
    cm, pm = SC.dome_mask(P)
    ba.set_constant(cm, pm)
    ba.checkpoint()
    b0, p0 = ba.cameras_bal(), ba.points()
    want_c, want_p = ba.constant()
    _use(ba)
    assert ba.filter_observations(t) == removed and 0 < removed < len(P["pt_idx"])
    assert _bits(ba.row_ptr, rows) and _bits(ba.pt_idx, pi) and _bits(ba.observations().reshape(-1, 2), uv.reshape(-1, 2))
    twin = _twin(c2b, ba, (cm, pm))
    assert np.abs(_same_state(ba, twin)).max() > 0.0
    got_c, got_p = ba.constant()
    assert _bits(got_c, want_c) and _bits(got_p, want_p) and want_c.any() and want_p.any()
    _checkpoint_in_force(env, ba, b0, p0)
    ba.close()
    twin.close()
