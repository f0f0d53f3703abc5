"""searchForTriangulation (k_tri_rays, k_tri_candidates, k_excl_scan and the loop over the candidate lists) and the
search of fuse (k_prepare_points' fuse mode, one k_match_round) on the device, against the library's sequential
host loops and the restatements of deftri.matching, and the chain search_for_triangulation -> triangulate -> fuse
-> localBundleAdjustment end to end.

Matches, statuses, distances and counters are integers: equal, on scenes whose fp64 restatement decides no
epipolar test of a pair with dist <= 50 within rel 1e-3 of epipolar_th (essential_scenes.near_threshold's margin)
and, for the search of fuse, nothing within projection_scenes.margins_ok's margins; the projections are held to
0.005 px of the fp64 restatement, the existing bar for this projection."""
import copy
import statistics
import time

import numpy as np
import pytest

from deftri import ba, capi, matching
from deftri.mapmodel import MapPoint
import projection_scenes as ps
import triangulation_matching_scenes as tm
from triangulation_matching_scenes import COUNTERS, same

gpu = pytest.mark.gpu
# one more keypoint than a wave's step over frame 2, and rows beyond one workgroup's four
SHAPES = [(64, 64), (65, 63), (63, 257), (257, 257)]


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


def three_way(gpu_ctx, host, s, flag_quirk, round_trips=1):
    """Device, host-only context and both restatements agree; returns the device's result."""
    r64 = tm.ref(s, flag_quirk, np.float64)
    assert tm.near_threshold(s, r64) == 0                                  # the builder kept every case
    got, want = gpu_ctx.search_for_triangulation(*tm.args(s, flag_quirk)), host.search_for_triangulation(*tm.args(s, flag_quirk))
    for k in ("matches", "best_dist", "status"):
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=k)
    assert got.n_matches == want.n_matches and all(got.report[k] == want.report[k] for k in COUNTERS)
    same(got, r64)
    same(got, tm.ref(s, flag_quirk))
    assert got.report["round_trips"] == round_trips
    return got


@gpu
@pytest.mark.parametrize("n1,n2", SHAPES)
@pytest.mark.parametrize("flag_quirk", [True, False])
def test_cloud_scenes(gpu_ctx, host, n1, n2, flag_quirk):
    s = tm.cloud_scene(n1, n2, seed=n1 + n2)
    assert len(s["uv1"]) == n1 and len(s["uv2"]) == n2
    got = three_way(gpu_ctx, host, s, flag_quirk)
    print(f"{n1} x {n2} quirk {flag_quirk}: statuses {np.bincount(got.status, minlength=5)}, listed {got.report['n_listed']}, "
          f"flag row {got.report['flag_row']}")
    if not flag_quirk:                                                     # every planted pair, no distractor
        free = ~s["has1"] & (s["true2"] >= 0) & ~s["has2"][np.maximum(s["true2"], 0)]
        np.testing.assert_array_equal(got.matches[free], s["true2"][free])
        assert got.report["n_occupied"] > 0 and got.report["n_unmatched"] > 0
    elif got.report["flag_row"] >= 0:
        assert (got.status[got.report["flag_row"] + 1:][~s["has1"][got.report["flag_row"] + 1:]] == 4).all()


@gpu
@pytest.mark.parametrize("n1", [1, 255, 256, 257, 600])
def test_row_offsets_at_the_scan_chunk_boundaries(gpu_ctx, host, n1):
    """The rows' counts are scanned by one workgroup of 256 threads, a contiguous chunk each: one row, one row
    below, at and above 256, and 600 rows in chunks of 3 that leave threads idle.  The rows cycle over six lines
    against 40 keypoints on five of them, so the counts differ from row to row, every sixth row (no keypoint on its
    line) and every seventh (it holds a map point) lists nothing, and rows rob each other throughout."""
    rows = [(i % 6, 3 + (5 * i) % 47, i % 7 == 3) for i in range(n1)]
    keys = [(j % 5, 2 + (7 * j) % 53, j % 11 == 5) for j in range(40)]
    s = tm.line_scene(rows, keys)
    got = three_way(gpu_ctx, host, s, False)
    r = tm.ref(s, False)
    listed = (~s["has1"][:, None] & ~s["has2"][None, :] & (r["dist"] <= 49) & (r["err"] < s["epipolar_th"])).sum(1)
    assert got.report["n_listed"] == listed.sum() and (n1 == 1 or len(set(listed.tolist())) > 3)


@gpu
def test_row_with_more_than_64_candidates(gpu_ctx, host):
    s = tm.crowded_row_scene()
    r = tm.ref(s)
    d = r["dist"][0, :-1]
    assert len(d) > 64 and r["matches"][0] == np.nonzero(d == d.min())[0][-1] and r["matches"][1] == len(d)
    got = three_way(gpu_ctx, host, s, True)
    assert got.report["n_listed"] == len(d) + 1


@gpu
def test_every_pair_passes(gpu_ctx, host):
    """65 x 65 identical descriptors under E = 0: the lists carry n1 * n2 entries; row i is left keypoint 64 - i."""
    n = 65
    s = tm.identical_scene(n)
    r = tm.ref(s)
    assert (r["dist"] == 0).all() and (r["err"] < s["epipolar_th"]).all()
    np.testing.assert_array_equal(r["matches"], n - 1 - np.arange(n))
    got = three_way(gpu_ctx, host, s, True)
    assert got.report["n_listed"] == n * n


@gpu
def test_lists_beyond_the_first_buffer(gpu_ctx, host):
    """130 x 130 identical descriptors: 16900 pairs against the first buffer's 64 * 130 + 4096: a second, exact pass."""
    n = 130
    s = tm.identical_scene(n)
    got = three_way(gpu_ctx, host, s, True, round_trips=2)
    assert got.report["n_listed"] == n * n
    np.testing.assert_array_equal(got.matches, n - 1 - np.arange(n))


@gpu
@pytest.mark.parametrize("decreasing", [True, False])
@pytest.mark.parametrize("order", [None, "permuted"])
def test_steal_chains(gpu_ctx, host, decreasing, order):
    perm = None if order is None else np.random.default_rng(4).permutation(10)
    s = tm.chain_scene(decreasing, perm)
    got = three_way(gpu_ctx, host, s, True)
    assert got.n_matches == 2 and (order is not None or got.report["n_stolen"] == 8)
    print(decreasing, order, got.matches, got.status)


@gpu
def test_flag_quirk_modes(gpu_ctx, host):
    for first, quirk, n_matches in ((2, True, 1), (2, False, 6), (3, True, 6), (3, False, 6)):
        got = three_way(gpu_ctx, host, tm.quirk_scene(first), quirk)
        assert got.n_matches == n_matches and got.report["flag_row"] == (0 if first == 2 else -1)


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_fuse_search_margin_scenes(gpu_ctx, host, n):
    s = tm.fuse_scene(n, seed=n)
    r64 = tm.fuse_ref(s, np.float64)
    assert len(s["pos"]) == n and tm.fuse_margins_ok(s, r64)                # the builder kept every case
    got, want = gpu_ctx.fuse_search(*tm.fuse_args(s)), host.fuse_search(*tm.fuse_args(s))
    err = float(np.abs(got.uv - r64["uv"])[s["consider"]].max(initial=0.0))
    print(f"n {n}: status counts {np.bincount(got.status, minlength=7)}, max |uv - uv64| {err:.3g} px")
    for k in ("match", "status", "best", "second"):
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=k)
        np.testing.assert_array_equal(getattr(got, k), r64[k], err_msg=k + " (fp64)")
    for k in ("n_points", "n_matches", "n_no_candidates", "n_rejected", "n_undefined"):
        assert got.report[k] == want.report[k] == r64["report"][k], k
    assert err < 0.005
    assert got.report["rounds"] == 1 and got.report["round_trips"] == 1
    if n >= 63:
        assert all((got.status == k).any() for k in (0, 3, 4, 6))


@gpu
def test_fuse_search_more_than_64_candidates(gpu_ctx, host):
    s = tm.crowded_fuse_scene()
    r = tm.fuse_ref(s, np.float64)
    cand = matching.features_in_area(s["grid"], matching.build_grid(s["grid"], s["uv2"]), s["uv2"], s["octave2"], r["uv"][0, 0],
                                     r["uv"][0, 1], r["radius"][0], 6, 8)
    assert len(cand) > 64
    got, want = gpu_ctx.fuse_search(*tm.fuse_args(s)), host.fuse_search(*tm.fuse_args(s))
    for k in ("match", "status", "best", "second"):
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=k)
        np.testing.assert_array_equal(getattr(got, k), r[k], err_msg=k)
    np.testing.assert_array_equal(got.match, [70, 80, 90])                 # no slot is skipped: all three are accepted


def grow_map(ctx, m, positions, grid):
    """The sequence on `ctx`: match keyframes 0 and 1, new map points at `positions` (one per row), fuse them into
    keyframe 2 (add branch), then fuse duplicates seen from keyframe 3 into keyframe 2 (fuse branch).  Returns (matches,
    n added, n fused, the ids of the duplicates)."""
    kf0, kf1, kf2, kf3 = (m.keyframes[k] for k in range(4))
    n = kf0.n_slots
    E = matching.essential_from_poses(kf1.pose, kf0.pose)                  # ray2 . (E ray1) = 0 for this formula
    matches, rep = matching.search_for_triangulation(ctx, kf0, kf1, 50, tm.EPI_TH, E=E, flag_quirk=False)
    assert rep["n_matches"] == n
    pts = []
    for i in range(n):
        mp = MapPoint(positions[i], pid=i)
        m.insert_map_point(mp)
        tm.observe(m, 0, mp, i)
        tm.observe(m, 1, mp, int(matches[i]))
        pts.append(mp)
    assert (m.update_orientation_and_descriptor(ctx, grid=grid) == 0).all()
    n_added, _ = matching.fuse(ctx, m, kf2, 50, pts, grid)
    dups = []
    for i in range(n):
        mp = MapPoint(positions[i], pid=1000 + i)
        m.insert_map_point(mp)
        tm.observe(m, 3, mp, i)
        dups.append(mp)
    assert (m.update_orientation_and_descriptor(ctx, [mp.id for mp in dups], grid) == 0).all()
    n_fused, _ = matching.fuse(ctx, m, kf2, 50, dups, grid)
    return matches, n_added, n_fused, [mp.id for mp in dups]


@gpu
def test_grow_a_map_end_to_end(gpu_ctx, host):
    n = 150
    grid = dict(ps.GRID)
    m, world = tm.four_views(n)
    kf0, kf1 = m.keyframes[0], m.keyframes[1]
    E = matching.essential_from_poses(kf1.pose, kf0.pose)
    free = np.zeros(n, bool)
    r = matching.search_for_triangulation_ref(kf0.keypoints, kf0.descriptors, free, kf1.keypoints, kf1.descriptors, free, kf0.kb8, E,
                                              50, tm.EPI_TH, flag_quirk=False)
    np.testing.assert_array_equal(r["matches"], np.arange(n))              # by construction, on the restatement first
    assert matching.search_for_triangulation_ref(kf0.keypoints, kf0.descriptors, free, kf1.keypoints, kf1.descriptors, free,
                                                 kf0.kb8, E, 50, tm.EPI_TH, flag_quirk=True)["n_matches"] < n
    x1, _, valid = gpu_ctx.triangulate(kf0.keypoints, kf1.keypoints, kf0.kb8, kf1.kb8, kf0.pose, kf1.pose)
    # 0.1 px of noise at f = 458 px and a baseline of 8 cm puts sigma_z = z^2 / (f b) * 0.14 px = 0.4 mm at z = 0.32 m
    print("max |x1 - world|", np.abs(x1 - world).max())
    assert valid.all() and np.abs(x1 - world).max() < 3e-3
    m_host = copy.deepcopy(m)
    matches, n_added, n_fused, dup_ids = grow_map(gpu_ctx, m, x1, grid)
    np.testing.assert_array_equal(matches, np.arange(n))
    assert n_added == n and n_fused == n                                   # every point gains the observation; every duplicate fuses
    assert len(m.map_points) == 2 * n - n_fused and not any(pid in m.map_points for pid in dup_ids)
    for i in range(n):                                                     # the survivors hold the union of the observations
        assert m.mp_obs[i] == {0: i, 1: i, 2: i, 3: i}
        assert all(m.keyframes[k].map_points[i] is m.map_points[i] for k in range(4))
    tm.check_map(m)
    assert grow_map(host, m_host, x1, grid)[1:3] == (n_added, n_fused)
    assert tm.map_signature(m_host) == tm.map_signature(m)
    rep = ba.localBundleAdjustment(m, 2)
    print("local BA:", rep["first"]["chi2_initial"], "->", rep["second"]["chi2_final"], "outliers", rep["outliers_removed"])
    assert np.isfinite(rep["second"]["chi2_final"])


@gpu
def test_times_at_2000_keypoints(gpu_ctx, host):
    """Prints the device call's and the host-only loop's milliseconds at n1 = n2 = 2000 (FeatureExtractor.nFeatures);
    asserts nothing about them."""
    s = tm.cloud_scene(2000, 2000, seed=3, rel=0.0)
    a = tm.args(s, False)
    out = {}
    for name, ctx in (("device", gpu_ctx), ("host", host)):
        r = ctx.search_for_triangulation(*a)                               # warm-up
        t = []
        for _ in range(7):
            t0 = time.perf_counter()
            r = ctx.search_for_triangulation(*a)
            t.append((time.perf_counter() - t0) * 1e3)
        out[name] = (statistics.median(t), min(t), max(t), r)
    d, h = out["device"], out["host"]
    np.testing.assert_array_equal(d[3].matches, h[3].matches)
    print(f"search_for_triangulation 2000 x 2000: device median {d[0]:.3f} ms (min {d[1]:.3f}, max {d[2]:.3f}; ms_device "
          f"{d[3].report['ms_device']:.3f}, ms_loop {d[3].report['ms_loop']:.3f}, listed {d[3].report['n_listed']}), host-only "
          f"loop median {h[0]:.3f} ms (min {h[1]:.3f}, max {h[2]:.3f}); matches {d[3].n_matches}")
