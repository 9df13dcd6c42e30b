"""The occlusion rays on the device held to exact geometry (tests/_occref.py), on ray families that work where the mesh
generator works: every point on a triangle, th ~ tfar.  Three routes: k_occlusion (device.occlusion_filter),
k_occlusion_bvh (device.OcclusionBVH.filter) and Level 1 (visibility_graph(triangles=...), with the caller's hierarchy,
and from the brute-force sweep).

The rule:
  * a ray the reference calls decided occluded is never kept, one it calls decided clear never dropped;
  * on every ray, open ones included, the all-triangles mask, the hierarchy mask, the float32 restatement and the C
    oracle's orc_occlusion_filter are equal bit for bit;
  * a LEAK -- a ray the geometry itself occludes (closed_exact) and the device keeps -- may only be an open ray.  Leaks
    are counted and printed, not forbidden: the triangle test is not watertight.  Most are rays whose only
    occluder is the triangle their own point lies on, met a hair inside tfar; those behind ANOTHER triangle (a seam, a
    grazed edge) are counted apart.

One line per family is printed (pytest -s): rays, decided / open shares, self-hits, leaks, brute != hierarchy."""
import numpy as np
import pytest

import _occref as R
import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c2b():
    import __graft_entry__ as entry
    entry.build()
    import city2ba_amd
    assert city2ba_amd.device_count() > 0
    return city2ba_amd


def level0(case):
    """(keep of k_occlusion, keep of k_occlusion_bvh) as bool arrays"""
    import torch
    from city2ba_amd import device as D
    dev = torch.device("cuda", 0)
    camblk = D.cameras_prepare_state(torch.from_numpy(case.cams).to(dev))
    pts4 = D.points_pad(torch.from_numpy(case.pts).to(dev))
    ci = torch.from_numpy(case.ci.astype(np.int32)).to(dev)
    pi = torch.from_numpy(case.pi.astype(np.int32)).to(dev)
    brute = torch.full((len(case.ci),), 7, dtype=torch.uint8, device=dev)
    D.occlusion_filter(camblk, pts4, ci, pi, torch.from_numpy(case.tri).to(dev), brute)
    bvh = D.OcclusionBVH(case.tri, dev)
    assert bvh.depth < 64 and sorted(bvh.order.tolist()) == list(range(len(case.tri)))
    hier = torch.full((len(case.ci),), 7, dtype=torch.uint8, device=dev)
    bvh.filter(camblk, pts4, ci, pi, hier)
    brute, hier = brute.cpu().numpy(), hier.cpu().numpy()
    assert set(np.unique(brute)) <= {0, 1} and set(np.unique(hier)) <= {0, 1}
    return brute == 1, hier == 1


def level1(c2b, case):
    """the rays Level 1 casts (the pairs its predicate keeps, as ray numbers of the case) and, per route, the rays it kept"""
    n_cam, n_pts = len(case.cams), len(case.pts)
    ba = c2b.BAProblem.from_visibility(case.cams, case.pts, np.zeros(n_cam + 1, dtype=np.uint64), [], np.zeros((0, 2)))

    def rays_of(row, pi):
        cam = np.repeat(np.arange(n_cam, dtype=np.int64), np.diff(row.astype(np.int64)))
        return cam * n_pts + pi.astype(np.int64)

    row0, pi0, _ = ba.visibility_graph(1e4)
    cast = rays_of(row0, pi0)
    _, keep = O.visibility_pairs(case.cams, case.pts, case.ci, case.pi, 1e4)
    assert np.array_equal(cast, np.nonzero(keep == 1)[0])                   # the oracle's predicate: the same pairs
    kept = {}
    for route, kw in (("library", {}), ("prebuilt", {"prebuilt_hierarchy": True}), ("dense", {"dense": True})):
        row, pi, _ = ba.visibility_graph(1e4, triangles=case.tri, **kw)
        kept[route] = rays_of(row, pi)
    ba.close()
    return cast, kept


@pytest.mark.parametrize("name", R.FAMILIES)
def test_family(c2b, name, capsys):
    tot = dict(rays=0, occluded=0, clear=0, open=0, self_hit=0, leaks=0, leaks_other=0, differ=0, cast=0)
    problems = []
    for case in R.family(name):
        v, closed = case.verdict, case.closed
        brute, hier = level0(case)
        keep_orc = O.occlusion_filter(case.cams, case.pts, case.ci, case.pi, case.tri) == 1
        tot["rays"] += len(brute)
        for k in ("occluded", "clear", "open", "self_hit"):
            tot[k] += int(v[k].sum())
        tot["differ"] += int((brute != hier).sum())
        leak = closed & brute
        tot["leaks"] += int(leak.sum())
        tot["leaks_other"] += int((leak & v["exact_other"]).sum())       # not merely the ray's own triangle at th ~ tfar
        for route, keep in (("k_occlusion", brute), ("k_occlusion_bvh", hier)):
            if keep[v["occluded"]].any():
                problems.append("%s %s: %d decided-occluded rays kept" % (case.name, route, keep[v["occluded"]].sum()))
            if not keep[v["clear"]].all():
                problems.append("%s %s: %d decided-clear rays dropped" % (case.name, route, (~keep[v["clear"]]).sum()))
            if not np.array_equal(keep, ~v["f32"]):
                problems.append("%s %s: %d rays differ from the restatement" % (case.name, route, (keep != ~v["f32"]).sum()))
        if not np.array_equal(keep_orc, ~v["f32"]):
            problems.append("%s: oracle differs from the restatement" % case.name)
        if not np.array_equal(brute, hier):
            problems.append("%s: brute != hierarchy on %d rays" % (case.name, (brute != hier).sum()))
        if (leak & ~v["open"]).any():
            problems.append("%s: %d leaks on decided rays" % (case.name, (leak & ~v["open"]).sum()))
        # Level 1: the rays its predicate keeps (every point in front of a camera), through three routes
        cast, kept = level1(c2b, case)
        tot["cast"] += len(cast)
        want = cast[~v["f32"][cast]]
        for route, got in kept.items():
            if not np.array_equal(got, want):
                problems.append("%s Level 1 (%s): kept %d rays, the restatement keeps %d" % (case.name, route, len(got), len(want)))
                continue
            mask = np.zeros(len(brute), dtype=bool)
            mask[got] = True
            if mask[cast][v["occluded"][cast]].any() or not mask[cast][v["clear"][cast]].all():
                problems.append("%s Level 1 (%s): a decided ray answered wrongly" % (case.name, route))
    with capsys.disabled():
        n = tot["rays"]
        print("\n%-8s rays %6d  decided occluded %5.1f %%  decided clear %5.1f %%  open %5.1f %%  self-hits %5d  leaks %3d (%d behind another triangle)  "
              "brute != hierarchy %d  (Level 1 cast %d of them)"
              % (name, n, 100.0 * tot["occluded"] / n, 100.0 * tot["clear"] / n, 100.0 * tot["open"] / n, tot["self_hit"],
                 tot["leaks"], tot["leaks_other"], tot["differ"], tot["cast"]))
    assert tot["cast"] >= 0.3 * tot["rays"]                                  # Level 1 is not tested on a remnant
    assert not problems, "\n".join(problems)
    assert tot["differ"] == 0
