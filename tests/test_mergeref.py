"""tests/_mergeref.py on hand-built cases with the expected partners written out, and on the split dome that
tests/test_gpu_merge.py runs on the device: there the reference alone must undo the split without one false merge."""
import numpy as np

import _mergeref as M

X = np.array([0.25, -0.5, 0.125])
RADIUS, MAX_ERROR = 0.5, 1e-4


def _round(cams, pts, views, seen_at=None, radius=RADIUS, max_error=MAX_ERROR, held=None):
    pts = np.asarray(pts, dtype=np.float64)
    row_ptr, pt_idx, uv = M.observe(cams, pts if seen_at is None else seen_at, views)
    return M.one_round(cams, pts, row_ptr, pt_idx, uv, radius, max_error, held), (row_ptr, pt_idx, uv)


def test_a_twin_pair_merges_onto_the_lower_index_and_keeps_its_bits():
    cams = M.simple_cameras(4)
    r, _ = _round(cams, [X, X], [(0, 0), (1, 0), (2, 1), (3, 1)])
    assert r["partner"].tolist() == [1, 0] and r["status"].tolist() == [M.CHOSEN, M.CHOSEN]
    assert r["into"].tolist() == [0, 0] and r["merged"] == 1 and r["pt_idx"].tolist() == [0, 0, 0, 0]
    assert r["pts"].tobytes() == np.array([X, X]).tobytes()                     # m == a exactly, b keeps its bits
    assert r["counts"] == dict(none=0, chosen=2, unobserved=0, held=0)


def test_a_close_pair_that_shares_a_camera_does_not_merge():
    cams = M.simple_cameras(3)
    r, _ = _round(cams, [X, X], [(0, 0), (1, 0), (1, 1), (2, 1)])
    assert r["partner"].tolist() == [-1, -1] and r["status"].tolist() == [M.NONE, M.NONE] and r["merged"] == 0
    assert r["tested"] == 1 and r["rejected"] == 1


def test_a_nearer_candidate_that_misses_an_observation_gives_way_to_the_next():
    cams = M.simple_cameras(6)
    pts = [X, X + [1e-7, 0, 0], X + [1e-6, 0, 0]]
    seen_at = [X, X + [0.1, 0, 0], X]                            # point 1's pixels belong to a landmark 0.1 away: off by ~1e-2
    r, _ = _round(cams, pts, [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)], seen_at=seen_at)
    assert r["partner"].tolist() == [2, -1, 0] and r["status"].tolist() == [M.CHOSEN, M.NONE, M.CHOSEN]
    assert r["into"].tolist() == [0, 1, 0] and r["rejected"] == 2 and r["tested"] == 3
    assert r["pts"][0].tolist() == M.merge_position(np.asarray(pts[0]), np.asarray(pts[2]), 2, 2).tolist()
    assert r["pts"][0, 0] != X[0] and r["pts"][2].tolist() == (X + [1e-6, 0, 0]).tolist()


def test_a_chain_merges_its_closer_pair_first_and_the_third_point_in_round_two():
    cams = M.simple_cameras(6)
    pts = np.array([X, X + [1e-3, 0, 0], X + [2.5e-3, 0, 0]])
    views = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)]
    row_ptr, pt_idx, uv = M.observe(cams, pts, views)
    kw = dict(radius=2.2e-3, max_error=1e-2)
    r1 = M.one_round(cams, pts, row_ptr, pt_idx, uv, **kw)
    assert r1["partner"].tolist() == [1, 0, 1] and r1["into"].tolist() == [0, 0, 2] and r1["merged"] == 1      # c chose b, b chose a
    assert abs(r1["pts"][0, 0] - (X[0] + 0.5e-3)) < 1e-15
    r2 = M.one_round(cams, r1["pts"], row_ptr, r1["pt_idx"], uv, **kw)
    assert r2["partner"].tolist() == [2, -1, 0] and r2["status"].tolist() == [M.CHOSEN, M.UNOBSERVED, M.CHOSEN]
    assert r2["into"].tolist() == [0, 1, 0]
    assert abs(r2["pts"][0, 0] - (X[0] + 0.5e-3 + 2e-3 / 3)) < 1e-15          # na = 4, nb = 2: a third of the way
    out = M.merge(cams, pts, row_ptr, pt_idx, uv, rounds=5, **kw)
    assert out["per_round"] == [1, 1, 0] and out["rounds"] == 3 and out["merged"] == 2 and out["map"].tolist() == [0, 0, 0]
    assert out["pts"].tobytes() == r2["pts"].tobytes() and out["pt_idx"].tolist() == [0] * 6
    one = M.merge(cams, pts, row_ptr, pt_idx, uv, rounds=1, **kw)
    assert one["per_round"] == [1] and one["map"].tolist() == [0, 0, 2]


def test_equal_distances_go_to_the_lower_index():
    cams = M.simple_cameras(6)
    h = 2.0 ** -10
    pts = np.array([[-h, 0, 0], [0, 0, 0], [h, 0, 0]])
    r, _ = _round(cams, pts, [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)], radius=1.5 * h, max_error=1e-2)
    assert r["partner"].tolist() == [1, 0, 1] and r["into"].tolist() == [0, 0, 2]


def test_held_and_unobserved_points_are_skipped():
    cams = M.simple_cameras(5)
    held = np.array([0, 1, 0, 0], dtype=np.uint8)
    r, _ = _round(cams, [X, X, -X, -X], [(0, 0), (1, 1), (2, 2), (3, 2)], held=held)
    assert r["partner"].tolist() == [-1, -1, -1, -1]
    assert r["status"].tolist() == [M.NONE, M.HELD, M.NONE, M.UNOBSERVED] and r["merged"] == 0 and r["tested"] == 0
    assert r["counts"] == dict(none=2, chosen=0, unobserved=1, held=1)


def test_an_observation_behind_its_camera_rejects_the_pair():
    cams = M.simple_cameras(4, behind=(3,))
    r, _ = _round(cams, [X, X], [(0, 0), (1, 0), (2, 1), (3, 1)])
    assert r["partner"].tolist() == [-1, -1] and r["rejected"] == 1
    front, _ = _round(M.simple_cameras(4), [X, X], [(0, 0), (1, 0), (2, 1), (3, 1)])
    assert front["partner"].tolist() == [1, 0]                  # (the same pair in front of all four merges)


def test_a_nan_coordinate_rejects_the_pair():
    cams = M.simple_cameras(4)
    bad = X.copy()
    bad[1] = np.nan
    r, _ = _round(cams, [X, bad], [(0, 0), (1, 0), (2, 1), (3, 1)], seen_at=[X, X])
    assert r["partner"].tolist() == [-1, -1] and r["merged"] == 0 and r["tested"] == 0       # d2 is NaN: not even a candidate
    r, _ = _round(cams, [bad, bad], [(0, 0), (1, 0), (2, 1), (3, 1)], seen_at=[X, X])
    assert r["partner"].tolist() == [-1, -1]


def test_radius_zero_takes_exact_twins_and_distance_equal_to_the_radius_counts():
    cams = M.simple_cameras(4)
    r, _ = _round(cams, [X, X], [(0, 0), (1, 0), (2, 1), (3, 1)], radius=0.0)
    assert r["partner"].tolist() == [1, 0]
    h = 2.0 ** -8
    pts = np.array([[0, 0, 0], [h, 0, 0]])
    at, _ = _round(cams, pts, [(0, 0), (1, 0), (2, 1), (3, 1)], radius=h, max_error=1e-2)
    below, _ = _round(cams, pts, [(0, 0), (1, 0), (2, 1), (3, 1)], radius=np.nextafter(h, 0.0), max_error=1e-2)
    assert at["partner"].tolist() == [1, 0] and below["partner"].tolist() == [-1, -1]


def test_the_reference_undoes_the_split_dome_without_a_false_merge():
    import __graft_entry__ as entry
    entry.build()
    S = M.split_dome()
    P, n0 = S["P"], S["n_orig"]
    assert 0 in S["twin_of"] and len(S["twin_of"]) == 120 and len(S["both"]) > 80
    import oracle as O
    cams = O.camera_from_bal(P["bal9"])
    out = M.merge(cams, P["pts"], P["row_ptr"], P["pt_idx"], P["uv"], RADIUS, MAX_ERROR, rounds=2)
    d2 = M.distances2(P["pts"][:n0])
    print("MERGE REFERENCE split dome (seed %d): %d both halves seen, per round %s, %d pairs rejected, %d borderline; closest distinct points %.3g"
          % (S["split_seed"], len(S["both"]), out["per_round"], out["rejected"], out["borderline"], np.sqrt(d2[np.triu_indices(n0, 1)].min())))
    want = np.arange(len(P["pts"]))
    for a in S["both"]:
        want[S["twin_of"][a]] = a
    assert out["map"].tolist() == want.tolist()                  # every pair with both halves seen, and no other: zero false merges
    assert out["per_round"] == [len(S["both"]), 0] and out["borderline"] == 0
    assert out["pts"][:n0].tobytes() == P["pts"][:n0].tobytes()
    lost = np.array([a for a, b in S["twin_of"].items() if a not in S["both"]] + [-1])
    differs = out["pt_idx"] != S["orig_pt_idx"].astype(np.int64)
    assert np.isin(S["orig_pt_idx"][differs].astype(np.int64), lost).all()
