"""The references of tests/_errref.py judged on the CPU, before tests/test_gpu_error_sums_reference.py holds the device to
them: the exact scenes project to their integers under the double-precision oracle, the long-double power agrees with mpmath,
and the exact restatement of pow_tab (m2log_tab with its signed k on all of (2^-1000, 2^1000), exp_tab) stays within E / 2 --
the condition a correct implementation meets on its own, with as much room again for the device."""
import collections
import math

import mpmath as mp
import numpy as np
import pytest

import _errref as E
import oracle as O

SIZES = (1, 63, 64, 65, 191, 192, 193, 1023, 1024, 1025, 1535, 1536, 1537, 13825)


@pytest.mark.parametrize("layout", E.LAYOUTS)
def test_exact_scenes_project_to_their_integers_under_the_oracle(layout):
    for n in SIZES:
        s = E.scene(n, layout)
        assert s["cam_idx"].shape == s["pt_idx"].shape == (n,) and s["uv"].shape == s["proj"].shape == s["a"].shape == (n, 2)
        res = s["proj"] - s["uv"]
        assert np.array_equal(res, s["a"].astype(np.float64)) and np.array_equal(res, np.rint(res))
        assert np.array_equal(s["uv"] * 8, np.rint(s["uv"] * 8)) and np.abs(s["a"]).max() <= 128
        if layout == "permuted":                               # the same observations as "rows", in another order
            rows = E.scene(n, "rows")
            assert sorted(map(tuple, np.column_stack([s["cam_idx"], s["pt_idx"]]))) == sorted(map(tuple, np.column_stack([rows["cam_idx"], rows["pt_idx"]])))
            assert n < 3 or not np.array_equal(s["cam_idx"], np.sort(s["cam_idx"]))
            row_ptr = np.arange(n + 1, dtype=np.uint64)        # the oracle takes rows: one observation per row, its camera repeated
            cams = s["cams15"][s["cam_idx"]]
        else:
            row_ptr, cams = s["row_ptr"].astype(np.uint64), s["cams15"]
            assert np.array_equal(np.repeat(np.arange(s["n_cam"]), np.diff(s["row_ptr"])), s["cam_idx"])
        got = O.project_observations(cams, s["pts"], row_ptr, s["pt_idx"].astype(np.uint64))
        assert np.array_equal(got.view(np.uint64), s["proj"].view(np.uint64)), (layout, n)
        l1, l2 = E.exact_sums(s["a"])
        assert 0 < l1 < 2 ** 53 and 0 < l2 < 2 ** 53
        assert O.total_reprojection_error(cams, s["pts"], row_ptr, s["pt_idx"].astype(np.uint64), s["uv"], 1.0) == float(l1)
        assert O.total_reprojection_error(cams, s["pts"], row_ptr, s["pt_idx"].astype(np.uint64), s["uv"], 2.0) == math.pow(float(l2), 0.5)


def test_scene_layouts_have_the_shapes_they_are_for():
    s = E.scene(1537, "rows")
    counts = np.diff(s["row_ptr"])
    assert set(E.DOME_LENGTHS) <= set(counts.tolist()) and counts[0] == 0
    runs = "".join("0" if c == 0 else "x" for c in counts)
    assert "000" in runs                                       # runs of empty rows ...
    assert any(np.searchsorted(s["row_ptr"], 64 * t, "left") + 3 < np.searchsorted(s["row_ptr"], 64 * t + 63, "right") for t in range(4))   # ... inside a tile
    one = E.scene(1537, "singles")
    assert one["n_cam"] == 1537 and np.array_equal(one["cam_idx"], np.arange(1537))        # 64 cameras per wave: more than kCamW = 12
    assert E.scene(5, "one")["n_cam"] == 1
    # every workgroup's share of either sum is positive, so a dropped or doubled partial changes it
    big = E.scene(1536 * 9 + 1, "one")
    per = np.add.reduceat(np.abs(big["a"]).sum(axis=1), np.arange(0, len(big["a"]), 1024))
    assert per.min() > 0
    # the largest list any test sums stays far below 2^53
    assert 2 * 128 ** 2 * (1536 * 2561 + 1) < 2 ** 53


def test_prefix_sums_are_the_sums_of_the_prefixes():
    s = E.scene(3000, "one")
    S1, S2 = E.exact_prefix_sums(s["a"])
    for n in (0, 1, 64, 1537, 3000):
        assert (int(S1[n]), int(S2[n])) == E.exact_sums(s["a"][:n])


def test_long_double_power_agrees_with_mpmath():
    mp.mp.dps = 60
    worst = 0.0
    for a, y, _ in E.pow_sample()[::5] + [(1e-300, 1.5, ""), (3.0, 0.5, ""), (2.0 ** -700, 1.5, "")]:
        got = E.term_ref(a, y)
        want = mp.power(mp.mpf(a), mp.mpf(y))
        if not mp.mpf(2) ** -16000 < want < mp.mpf(2) ** 16000:    # beyond the long double's own range (far beyond the double's)
            assert got == 0 or np.isinf(got)
            continue
        m, ex = np.frexp(got)
        got_mp = mp.ldexp(mp.mpf(int(np.ldexp(m, 64))), int(ex) - 64)      # the long double's 64 bits, exactly
        worst = max(worst, float(abs(got_mp - want) / want))
    assert worst <= 2.0 ** -60, worst


def test_m2log_split_handles_every_exponent():
    for x, want_k in ((1.0, 0), (0.6875, 0), (1.375, 1), (math.nextafter(1.375, 0.0), 0), (2.0 ** -999, -999), (2.0 ** 999, 999),
                      (1.5 * 2.0 ** -999, -998), (1.3 * 2.0 ** 40, 40), (0.7 * 2.0 ** -40, -40)):
        z, k, i = E.m2log_split(x)
        assert k == want_k and 0.6875 <= z < 1.375 and math.ldexp(z, k) == x and 0 <= i < 128, (x, z, k, i)
    assert E.m2log_split(1.0)[2] == 80 and E.m2log_split(math.nextafter(1.0, 0.0))[2] == 79


def test_logarithm_restated_exactly_holds_its_ulps_on_all_of_its_domain():
    """-2 ln x with 53-bit arguments and signed k (tests/test_noise_tables.py: 32-bit u in (0, 1] only): a few ulps"""
    mp.mp.dps = 40
    worst = 0.0
    for a, _, tag in E.pow_sample():
        if tag == "exps" and not (2.0 ** -1000 < a < 2.0 ** 1000) or a == 1.0:
            continue
        got, want = E.m2log_tab_exact(a), -2 * mp.log(mp.mpf(a))
        worst = max(worst, float(abs(mp.mpf(got) - want) / abs(want)) / E.U)
    assert E.m2log_tab_exact(1.0) == 0.0
    assert worst <= 4.0, worst                               # in units of 2^-53 relative: two ulps


def test_pow_tab_restated_exactly_stays_within_half_its_bound():
    sample = E.pow_sample()
    assert 3000 < len(sample) < 6000
    worst, at = collections.defaultdict(float), {}
    fallback = collections.Counter()
    for a, y, tag in sample:
        r = E.restatement_ratio(a, y)
        if r is None:
            fallback[(tag, y)] += 1
            continue
        for key in (tag, y, "all"):
            if r > worst[key]:
                worst[key], at[key] = r, (a, y)
    print("\nWORST |pow_tab_exact - ref| / ((|y ln a| + 1) 2^-53 |a|^y): %.3f at %r; C = %g" % (worst["all"], at["all"], E.C))
    print("  per class: " + ", ".join("%s %.3f" % (k, worst[k]) for k in ("sizes", "near1", "ends", "exps", "edge")))
    print("  per norm:  " + ", ".join("%g %.3f" % (k, worst[k]) for k in E.NORMS))
    print("  library fallback: " + ", ".join("%s/%g x%d" % (t, y, c) for (t, y), c in sorted(fallback.items())))
    assert worst["all"] <= E.C / 2                           # within E / 2 in every case
    assert E.C <= 2.2 * worst["all"]                         # ... and C is the measurement doubled, not a guess
    # which arguments take the library's pow: everything outside (2^-1000, 2^1000) and |y ln a| >= 600, nothing else
    for a, y, tag in sample:
        l = y * math.log(a)
        outside = not (2.0 ** -1000 < a < 2.0 ** 1000)
        assert E.pow_tab_fallback(a, y) == (outside or abs(l) >= 600.0) or abs(abs(l) - 600.0) < 1e-9, (a, y, tag)
    assert fallback[("sizes", 30.0)] > 0 and not any(fallback[("sizes", y)] for y in E.NORMS if y != 30.0)
    assert not any(fallback[("near1", y)] for y in E.NORMS)
    assert all(fallback[("edge", y)] == 2 for y in E.NORMS if y >= 1.25)     # the two arguments at 600.1
    assert E.pow_tab_exact(1.5 * 2.0 ** 999, 0.5) is not None and E.pow_tab_exact(1.5 * 2.0 ** -999, 0.1) is not None
    assert E.pow_tab_exact(1.0, 7.3) == 1.0


@pytest.mark.parametrize("mutation", E.MUTATIONS)
def test_the_logarithms_arithmetic_mutations_leave_the_bound(mutation):
    """-2/3 shortened to four digits, kd dropped from `tail`: in the restatement each lands outside E (not E / 2) in the sample"""
    ratios = [E.restatement_ratio(a, y, mutation) for a, y, _ in E.pow_sample() if y in (1.5, 7.3)]
    bad = [r for r in ratios if r is not None and r > E.C]
    print("\n%s: %d of %d sampled arguments outside E, worst ratio %.3g" % (mutation, len(bad), len(ratios), max(bad)))
    assert len(bad) > 20


def test_depth_counts_the_longest_path():
    assert E.launch_grid(1, E.LIGHT_SHAPE) == 1 and E.launch_grid(1536, E.LIGHT_SHAPE) == 1 and E.launch_grid(1537, E.LIGHT_SHAPE) == 2
    assert E.launch_grid(1024 * 1537, E.JAC_SHAPE) == 1537
    assert E.device_depth(1) == 6 + 6 + 8 + 3 + 6 + 8
    assert E.device_depth(1536 * 512 + 1) == E.device_depth(1) + 1        # the 513th workgroup: a second partial on thread 0
    assert E.device_depth(1536 * 2561) == E.device_depth(1) + 5
    assert E.device_depth(1024 * 1024 + 1, E.JAC_SHAPE) == 2 + 6 + 16 + 4 + 6 + 16


def test_sum_bound_holds_for_plain_double_sums_of_the_same_depth():
    """terms from the restatement, summed in f64 in two orders whose depth is known (sequential: n; pairwise halving: log2 n)"""
    rng = np.random.default_rng(8)
    a = 10.0 ** rng.uniform(-12, 3, 512)
    for y in (0.5, 1.25, 3.0, 7.3):
        t = np.array([E.pow_tab_exact(v, y) for v in a])
        ref = E.term_ref(a, y).sum()
        e_terms, total = float(E.term_bound(a, y).sum()), float(ref)
        seq = 0.0
        for v in t:
            seq += v
        tree = t.copy()
        while len(tree) > 1:
            tree = tree[0::2] + tree[1::2]
        assert abs(E.LD(seq) - ref) <= e_terms + 512 * E.U * total
        assert abs(E.LD(tree[0]) - ref) <= e_terms + 9 * E.U * total
