"""The error sums sum |du|^norm + |dv|^norm on every route that computes them -- k_observations<MODE_ERROR | MODE_ERROR12 |
MODE_NOISE_ERROR12>, k_residual_jacobian_l<.., WITH_ERR>, ticket_fold_n, Level 1 -- against the references of tests/_errref.py
(judged on the CPU by tests/test_errref.py):

  * exact-integer scenes: the sums must EQUAL Python ints, at every lane / tile / wave / workgroup edge, at the leaf counts of
    ticket_arrive and around the four-chain loop of the last arriver's fold;
  * one term per launch: the sum IS one pow_tab (light route) or pow_lean (fused Jacobian) value, held to E(a, y), and the same
    term at chosen positions of a list of zero residuals must give the same bits;
  * general sums with residuals of 15 orders of magnitude and of one magnitude each, held to the sum bound;
  * a NaN or an infinity among the observations reaches every sum.

The worst ratios are printed (run with -s) and recorded in DESIGN.md, "What the error sums' tests cover"."""
import math

import numpy as np
import pytest

import _errref as E
from _problems import dome_problem, random_problem

pytestmark = pytest.mark.gpu

SMALL = (1, 63, 64, 65, 191, 192, 193, 1023, 1024, 1025, 1535, 1536, 1537)
GRIDS = (8, 9, 15, 63, 64, 65, 128, 129)                    # xcd_tile32's remainders, ticket_arrive's leaves
FOLD_GRIDS = (511, 512, 513, 1536, 1537, 2047, 2048, 2049, 2561)      # k + 3 * step < n, step 512 (light routes)
JAC_GRIDS = GRIDS + (511, 512, 513)                         # workgroups of 1 024 observations: n <= 600 000
JAC_FOLD_GRIDS = (1537, 3073)                               # past 1 536 partials; past 3 * 1 024: the four-chain loop at step 1 024
N_LIGHT = 1536 * max(FOLD_GRIDS) + 1
N_JAC = 1024 * max(JAC_FOLD_GRIDS) + 1
# True: the device's pow_tab values on the table route equal tests/_errref.py's exact restatement bit for bit (the first run on
# the MI355X showed no difference); the bound E is asserted as well
ASSERT_TABLE_BITS = True


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build()
    import torch
    import city2ba_amd
    from city2ba_amd import device as D
    assert city2ba_amd.device_count() > 0, "no HIP device: the gpu tests must run on the GPU box"
    dev = torch.device("cuda", 0)
    return dict(torch=torch, c2b=city2ba_amd, D=D, dev=dev, ws=D.workspace(max(N_LIGHT, N_JAC), dev))


class Lists:
    """a problem's tables and observation lists on the device; `rows` is made per call (a prefix of one camera's list is a list)"""

    def __init__(self, env, cams15, pts, cam_idx, pt_idx, uv, row_ptr=None):
        torch, D, dev = env["torch"], env["D"], env["dev"]
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
        self.env, self.n = env, len(cam_idx)
        self.camblk = D.cameras_prepare_state(up(cams15, np.float64))
        self.pts4 = D.points_pad(up(pts, np.float64))
        self.ci, self.pi, self.uv = up(cam_idx, np.int32), up(pt_idx, np.int32), up(uv, np.float64)
        self.row_ptr = None if row_ptr is None else up(row_ptr, np.int64)
        self.one_camera = row_ptr is not None and len(row_ptr) == 2

    def rows(self, n):
        D, torch = self.env["D"], self.env["torch"]
        if self.row_ptr is None:
            return None
        if n == self.n:
            return D.Rows(self.row_ptr, n)
        assert self.one_camera
        return D.Rows(torch.tensor([0, n], dtype=torch.int64, device=self.env["dev"]), n)

    def project(self, n=None):
        n = self.n if n is None else n
        out = self.env["torch"].full((n, 2), 7.0, dtype=self.env["torch"].float64, device=self.env["dev"])
        return self.env["D"].project(self.camblk, self.pts4, self.ci[:n], self.pi[:n], out)


def light_sums(T, n, norms, uv=None, fused=True):
    """{route: value} of every light route over the first n observations: the cam_idx and the rows form per norm, the L1 / L2 pair
    in one pass, and the fused observation noise at std 0 (which must leave uv's bits alone)"""
    env = T.env
    torch, D, ws = env["torch"], env["D"], env["ws"]
    uv = T.uv if uv is None else uv
    rows = T.rows(n)
    names, out = [], torch.full((2 * len(norms) + 4,), -1.0, dtype=torch.float64, device=env["dev"])
    k = 0
    for y in norms:
        D.reprojection_error_sum(T.camblk, T.pts4, T.ci[:n], T.pi[:n], uv[:n], y, ws, out[k:k + 1])
        names.append("sum/idx/%g" % y)
        k += 1
        if rows is not None:
            D.reprojection_error_sum_rows(T.camblk, T.pts4, rows, T.pi[:n], uv[:n], y, ws, out[k:k + 1])
            names.append("sum/rows/%g" % y)
            k += 1
    if rows is not None:
        D.reprojection_error_sums2_rows(T.camblk, T.pts4, rows, T.pi[:n], uv[:n], ws, out[k:k + 2])
        names += ["sums2/rows/1", "sums2/rows/2"]
        k += 2
        if fused:
            mine = uv[:n].clone()
            D.add_noise_observations_error_sums2_rows(T.camblk, T.pts4, rows, T.pi[:n], mine, 0, 0.0, 99, ws, out[k:k + 2])
            names += ["noise0/rows/1", "noise0/rows/2"]
            k += 2
            if not bool(torch.isnan(uv[:n]).any().item()):
                assert torch.equal(mine.view(torch.int64), uv[:n].view(torch.int64)), "the fused noise pass at std 0 changed uv (n = %d)" % n
    return dict(zip(names, out[:k].cpu().numpy().tolist()))


class JacOut:
    def __init__(self, env, n):
        torch, dev = env["torch"], env["dev"]
        self.r, self.Jc, self.Jp = (torch.full((n, w), 5.0, dtype=torch.float64, device=dev) for w in (2, 18, 6))


def jac_sums(T, n, norms, J, uv=None, want_r=None):
    """{route: value} of the fused Jacobian's sum over the first n observations, cam_idx and rows form; want_r [>= n, 2] (device):
    the residuals both must write, bit for bit"""
    env = T.env
    torch, D, ws = env["torch"], env["D"], env["ws"]
    uv = T.uv if uv is None else uv
    rows = T.rows(n)
    names, out = [], torch.full((2 * len(norms),), -1.0, dtype=torch.float64, device=env["dev"])
    k = 0
    for y in norms:
        D.residual_jacobian_sum(T.camblk, T.pts4, T.ci[:n], T.pi[:n], uv[:n], J.r[:n], J.Jc[:n], J.Jp[:n], y, ws, out[k:k + 1])
        names.append("jac/idx/%g" % y)
        k += 1
        if want_r is not None:
            assert torch.equal(J.r[:n].view(torch.int64), want_r[:n].view(torch.int64)), "jac/idx: r (n = %d)" % n
        if rows is not None:
            J.r[:n].fill_(5.0)
            D.residual_jacobian_rows(T.camblk, T.pts4, rows, T.pi[:n], uv[:n], J.r[:n], J.Jc[:n], J.Jp[:n], norm=y, ws=ws, out_sum=out[k:k + 1])
            names.append("jac/rows/%g" % y)
            k += 1
            if want_r is not None:
                assert torch.equal(J.r[:n].view(torch.int64), want_r[:n].view(torch.int64)), "jac/rows: r (n = %d)" % n
    return dict(zip(names, out[:k].cpu().numpy().tolist()))


def _check_exact(got, l1, l2, label):
    assert 0 < l1 < 2 ** 53 and 0 < l2 < 2 ** 53
    bad = ["%s %s: %r, exactly %d" % (label, name, v, l1 if name.endswith("/1") else l2)
           for name, v in got.items() if v != float(l1 if name.endswith("/1") else l2)]
    assert not bad, "\n".join(bad)


# ---- exact sums ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_camera(env):
    """layout "one" at the largest size any test sums; every smaller size is a prefix.  Precondition: project() returns the integers"""
    torch, dev = env["torch"], env["dev"]
    s = E.scene(max(N_LIGHT, N_JAC), "one")
    T = Lists(env, s["cams15"], s["pts"], s["cam_idx"], s["pt_idx"], s["uv"], s["row_ptr"])
    want = torch.from_numpy(s["proj"]).to(dev)
    assert torch.equal(T.project().view(torch.int64), want.view(torch.int64)), "project() does not return the scene's integers bit for bit"
    S1, S2 = E.exact_prefix_sums(s["a"])
    return dict(T=T, S1=S1, S2=S2, a=torch.from_numpy(s["a"].astype(np.float64)).to(dev))


def test_exact_sums_at_lane_tile_wave_workgroup_and_leaf_edges(env, one_camera):
    T, S1, S2 = one_camera["T"], one_camera["S1"], one_camera["S2"]
    for n in SMALL + tuple(1536 * g + d for g in GRIDS for d in (-1, 0, 1)):
        _check_exact(light_sums(T, n, (1.0, 2.0)), int(S1[n]), int(S2[n]), "n = %d" % n)


def test_exact_sums_around_the_four_chains_of_the_last_arrivers_fold(env, one_camera):
    """grids of 511 .. 2 561 workgroups of 512 threads: a thread's second partial, the first trip of the four-chain loop (1 537),
    its last thread (2 048), the remainder loop behind it (2 049), a second trip with a remainder (2 561)"""
    T, S1, S2 = one_camera["T"], one_camera["S1"], one_camera["S2"]
    # the largest list first: every partial slot a smaller grid could wrongly read then holds a positive integer, not whatever
    # the allocation came with
    for n in (N_LIGHT,) + tuple(1536 * g + d for g in FOLD_GRIDS for d in (-1, 0, 1)):
        assert E.launch_grid(n, E.LIGHT_SHAPE) == -(-n // 1536)
        _check_exact(light_sums(T, n, (1.0, 2.0)), int(S1[n]), int(S2[n]), "n = %d" % n)


def test_exact_sums_of_the_fused_jacobian(env, one_camera):
    """r must be the integers; workgroups of 1 024 observations up to 600 000, then one grid past 1 536 partials and one past
    3 072 (the four-chain loop at step 1 024)"""
    T, S1, S2 = one_camera["T"], one_camera["S1"], one_camera["S2"]
    J = JacOut(env, N_JAC)
    light_sums(T, 1536 * 2049, (1.0,), fused=False)          # partial slots up to 2 * 2 049 hold positive integers (see above)
    sizes = SMALL + tuple(1536 * g + d for g in GRIDS for d in (-1, 0, 1)) + tuple(1024 * g + d for g in JAC_GRIDS for d in (-1, 0, 1))
    assert max(sizes) <= 600000
    for n in sizes + tuple(1024 * g + 1 for g in JAC_FOLD_GRIDS):
        _check_exact(jac_sums(T, n, (1.0, 2.0), J, want_r=one_camera["a"]), int(S1[n]), int(S2[n]), "n = %d" % n)


@pytest.mark.parametrize("layout", ["rows", "singles", "permuted"])
def test_exact_sums_of_the_other_camera_layouts(env, layout):
    torch, dev = env["torch"], env["dev"]
    J = JacOut(env, 1536 * 9 + 1)
    for n in SMALL + (1536 * 9 + 1,):
        s = E.scene(n, layout)
        T = Lists(env, s["cams15"], s["pts"], s["cam_idx"], s["pt_idx"], s["uv"], s["row_ptr"])
        assert torch.equal(T.project().view(torch.int64), torch.from_numpy(s["proj"]).to(dev).view(torch.int64)), "project(): %s %d" % (layout, n)
        l1, l2 = E.exact_sums(s["a"])
        a = torch.from_numpy(s["a"].astype(np.float64)).to(dev)
        _check_exact(light_sums(T, n, (1.0, 2.0)), l1, l2, "%s n = %d" % (layout, n))
        _check_exact(jac_sums(T, n, (1.0, 2.0), J, want_r=a), l1, l2, "%s n = %d" % (layout, n))


@pytest.mark.parametrize("layout,n", [("one", 1), ("one", 1537), ("one", 1536 * 513 + 1), ("rows", 1537), ("rows", 1536 * 9 + 1),
                                      ("singles", 1537), ("singles", 1536 * 9 + 1)])
def test_exact_sums_through_level_1(env, layout, n):
    """total_reprojection_error = the host's pow(sum, 1 / norm) of the exact sum"""
    s = E.scene(n, layout)
    ba = env["c2b"].BAProblem.from_visibility(s["cams15"], s["pts"], s["row_ptr"].astype(np.uint64), s["pt_idx"].astype(np.uint64), s["uv"])
    l1, l2 = E.exact_sums(s["a"])
    assert ba.total_reprojection_error(1.0) == math.pow(float(l1), 1.0 / 1.0)
    assert ba.total_reprojection_error(2.0) == math.pow(float(l2), 1.0 / 2.0)
    assert ba.total_reprojection_errors_l1_l2() == (math.pow(float(l1), 1.0), math.pow(float(l2), 0.5))


# ---- one term per launch -----------------------------------------------------------------------------------------------
def _term_args():
    """about 1 500 of the CPU sample's (a, y): a quarter of the sizes, half of the arguments near 1, every edge"""
    by = {}
    for s in E.pow_sample():
        by.setdefault(s[2], []).append(s)
    return by["sizes"][::4] + by["near1"][::2] + by["ends"] + by["exps"] + by["edge"]


def _term_scene(env, n=1):
    """one camera (R = I, t = (1, 0, 0), f = 1) and one point (-1, 0, -1): every observation projects to (0, 0), so the
    residual is -uv exactly"""
    cams15 = np.zeros((1, 15))
    cams15[0, [0, 4, 8, 9, 12]] = 1.0
    T = Lists(env, cams15, np.array([[-1.0, 0.0, -1.0]]), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros((n, 2)), np.array([0, n]))
    assert bool((T.project() == 0.0).all().item())
    return T


def _one_term_values(env, args, route):
    torch, D, ws, dev = env["torch"], env["D"], env["ws"], env["dev"]
    T = _term_scene(env)
    uv = torch.from_numpy(np.array([[-a, 0.0] for a, _, _ in args])).to(dev)
    out = torch.full((len(args),), -1.0, dtype=torch.float64, device=dev)
    J = JacOut(env, 1)
    for i, (_, y, _) in enumerate(args):
        if route == "light":
            D.reprojection_error_sum(T.camblk, T.pts4, T.ci, T.pi, uv[i:i + 1], y, ws, out[i:i + 1])
        else:
            D.residual_jacobian_sum(T.camblk, T.pts4, T.ci, T.pi, uv[i:i + 1], J.r, J.Jc, J.Jp, y, ws, out[i:i + 1])
    return out.cpu().numpy()


@pytest.mark.parametrize("route", ["light", "jacobian"])
def test_one_term_per_launch_against_the_long_double_power(env, route):
    """n = 1, dv = 0: the launch's sum is pow_tab(|du|, norm) (light) or pow_lean(|du|, norm) (fused Jacobian), bit for bit"""
    args = _term_args()
    assert 1400 <= len(args) <= 1700
    got = _one_term_values(env, args, route)
    msgs, worst, at, differ, table_route = [], 0.0, None, [], 0
    for (a, y, tag), v in zip(args, got):
        ref = E.term_ref(a, y)
        cls = E.value_class(np.float64(ref))
        if cls != "normal":
            if E.value_class(v) != cls:
                msgs.append("%s a = %r y = %g: %r is not %s like the reference %r" % (tag, a, y, v, cls, float(ref)))
            continue
        ratio = float(abs(E.LD(v) - ref) / E.LD(E.term_bound(a, y))) if np.isfinite(v) else np.inf
        if ratio > worst:
            worst, at = ratio, (a, y, tag)
        if not ratio <= 1.0:
            msgs.append("%s a = %r y = %g: dev %r ref %r |err| / E = %.3g" % (tag, a, y, v, float(ref), ratio))
        if route == "light":
            exact = E.pow_tab_exact(a, y)
            if exact is not None:
                table_route += 1
                if exact != v:
                    differ.append((a, y, v, exact))
    print("\nWORST |dev - ref| / E  one term, %s route: %.3f at %r (C = %g)" % (route, worst, at, E.C))
    if route == "light":
        print("pow_tab values that differ from the exact restatement: %d of %d on the table route%s"
              % (len(differ), table_route, "" if not differ else "; first " + repr(differ[0])))
        if ASSERT_TABLE_BITS:
            assert not differ, differ[:5]
    assert not msgs, "\n".join(msgs[:20])


@pytest.mark.parametrize("route", ["light", "jacobian"])
def test_one_term_among_zero_residuals_gives_the_bits_of_the_single_term(env, route):
    """the term at the first and last lane of a tile, a wave's tile edges, a workgroup edge and the end of the list"""
    torch, D, ws, dev = env["torch"], env["D"], env["ws"], env["dev"]
    cases = [(a, y) for y in (0.5, 3.0) for a in (3.7e-7, 0.731, 123.4)]
    single = _one_term_values(env, [(a, y, "") for a, y in cases], route)
    assert np.all(single > 0) and np.all(np.isfinite(single))
    bad = []
    for n in (1537, 3073):
        T, J = _term_scene(env, n), JacOut(env, n)
        rows = T.rows(n)
        places = (0, 63, 64, 191, 192, 1535, 1536, n - 1)
        out = torch.full((len(cases), len(places), 2), -1.0, dtype=torch.float64, device=dev)
        for i, (a, y) in enumerate(cases):
            for j, k in enumerate(places):
                uv = torch.zeros((n, 2), dtype=torch.float64, device=dev)
                uv[k, 0] = -a
                if route == "light":
                    D.reprojection_error_sum(T.camblk, T.pts4, T.ci, T.pi, uv, y, ws, out[i, j, 0:1])
                    D.reprojection_error_sum_rows(T.camblk, T.pts4, rows, T.pi, uv, y, ws, out[i, j, 1:2])
                else:
                    D.residual_jacobian_sum(T.camblk, T.pts4, T.ci, T.pi, uv, J.r, J.Jc, J.Jp, y, ws, out[i, j, 0:1])
                    D.residual_jacobian_rows(T.camblk, T.pts4, rows, T.pi, uv, J.r, J.Jc, J.Jp, norm=y, ws=ws, out_sum=out[i, j, 1:2])
        got = out.cpu().numpy()
        for i, (a, y) in enumerate(cases):
            for j, k in enumerate(places):
                for f, form in enumerate(("idx", "rows")):
                    if got[i, j, f] != single[i]:
                        bad.append("n = %d place %d %s a = %r y = %g: %r, alone %r" % (n, k, form, a, y, got[i, j, f], single[i]))
    assert not bad, "\n".join(bad[:20])


# ---- general sums ------------------------------------------------------------------------------------------------------
GENERAL_NORMS = (0.5, 1.25, 3.0, 7.3)
BANDS = (None, 1e-12, 1e-6, 1.0, 1e3)                       # None: log-uniform in 1e-12 .. 1e3 per observation


def _general_problem(name):
    if name == "dome":
        return dome_problem()
    return random_problem(60, 6000, 100, seed=31, k_scale=1e-2)


@pytest.mark.parametrize("name", ["dome", "random"])
def test_general_sums_stay_inside_the_sum_bound(env, name):
    """k2 != 0 cameras, residuals scaled per observation over 15 orders of magnitude, and bands of one magnitude each.  The
    terms are taken from the device's own project() minus uv: one IEEE subtraction, the bits the kernels form."""
    torch, dev = env["torch"], env["dev"]
    P = _general_problem(name)
    assert np.count_nonzero(P["cams15"][:, 14]) > len(P["cams15"]) // 2
    counts = np.diff(P["row_ptr"].astype(np.int64))
    cam_idx = np.repeat(np.arange(len(counts)), counts)
    n = len(cam_idx)
    assert n > (1536 if name == "random" else 1024)            # more than one workgroup of either shape
    T = Lists(env, P["cams15"], P["pts"], cam_idx, P["pt_idx"].astype(np.int64), np.zeros((n, 2)), P["row_ptr"].astype(np.int64))
    proj = T.project().cpu().numpy()
    assert np.all(np.isfinite(proj))
    rng = np.random.default_rng(17)
    J = JacOut(env, n)
    worst = {"light": 0.0, "jac": 0.0}
    msgs = []
    for band in BANDS:
        size = 10.0 ** rng.uniform(-12.0, 3.0, n) if band is None else np.full(n, band)
        ang = rng.uniform(0.0, 2 * np.pi, n)
        uv = proj - size[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])
        res = proj - uv
        uv_d, res_d = torch.from_numpy(uv).to(dev), torch.from_numpy(res).to(dev)
        got = light_sums(T, n, GENERAL_NORMS, uv=uv_d, fused=False)
        got.update(jac_sums(T, n, GENERAL_NORMS, J, uv=uv_d, want_r=res_d))
        for y in GENERAL_NORMS:
            for kind, shape in (("light", E.LIGHT_SHAPE), ("jac", E.JAC_SHAPE)):
                ref, bound = E.sum_bound(res, y, shape)
                for route in ("sum/idx", "sum/rows") if kind == "light" else ("jac/idx", "jac/rows"):
                    v = got["%s/%g" % (route, y)]
                    ratio = float(abs(E.LD(v) - ref) / E.LD(bound)) if np.isfinite(v) else np.inf
                    worst[kind] = max(worst[kind], ratio)
                    if not ratio <= 1.0:
                        msgs.append("%s band %r norm %g %s: dev %r ref %r |err| / bound %.3g" % (name, band, y, route, v, float(ref), ratio))
    print("\nWORST |dev - ref| / sum bound  %s (%d observations): light %.3f, fused Jacobian %.3f" % (name, n, worst["light"], worst["jac"]))
    assert not msgs, "\n".join(msgs[:20])


# ---- non-finite values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_observation_reaches_every_sum(env, value):
    """one NaN (then one infinity) at the first, a middle and the last observation of 1 537: every route returns NaN (+inf) at
    every norm -- the LM loop's termination 4 relies on it"""
    torch, dev = env["torch"], env["dev"]
    n = 1537
    s = E.scene(n, "rows")
    T = Lists(env, s["cams15"], s["pts"], s["cam_idx"], s["pt_idx"], s["uv"], s["row_ptr"])
    J = JacOut(env, n)
    norms = (1.0, 2.0) + GENERAL_NORMS
    ok = (lambda v: v != v) if value != value else (lambda v: v == math.inf)
    bad = []
    for k, col in ((0, 0), (768, 1), (n - 1, 0)):
        uv = s["uv"].copy()
        uv[k, col] = value
        uv_d = torch.from_numpy(uv).to(dev)
        got = light_sums(T, n, norms, uv=uv_d)
        got.update(jac_sums(T, n, norms, J, uv=uv_d))
        ba = env["c2b"].BAProblem.from_visibility(s["cams15"], s["pts"], s["row_ptr"].astype(np.uint64), s["pt_idx"].astype(np.uint64), uv)
        for y in norms:
            got["level1/%g" % y] = ba.total_reprojection_error(y)
        got["level1/l1"], got["level1/l2"] = ba.total_reprojection_errors_l1_l2()
        bad += ["observation %d: %s = %r" % (k, name, v) for name, v in got.items() if not ok(v)]
    assert not bad, "\n".join(bad)
