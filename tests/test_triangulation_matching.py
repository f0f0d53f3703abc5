"""searchForTriangulation and fuse on a host-only context (the library's sequential loops) against the numpy
restatements of deftri.matching, and Map.fuse_map_points / remove_map_point.  Hand-built scenes
(triangulation_matching_scenes.line_scene): what is expected is asserted on the restatement first, then the
library must equal the restatement in every integer output and counter."""
import ctypes as C

import numpy as np
import pytest

from deftri import _abi, capi, matching
from deftri.mapmodel import MapPoint
import projection_scenes as ps
import triangulation_matching_scenes as tm

from triangulation_matching_scenes import same


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


def check(host, s, matches, status, n_matches, flag_quirk=True, best=None):
    r = tm.ref(s, flag_quirk)
    np.testing.assert_array_equal(r["matches"], matches)
    np.testing.assert_array_equal(r["status"], status)
    assert r["n_matches"] == n_matches
    if best is not None:
        np.testing.assert_array_equal(r["best_dist"], best)
    assert tm.near_threshold(s, tm.ref(s, flag_quirk, np.float64)) == 0
    got = host.search_for_triangulation(*tm.args(s, flag_quirk))
    same(got, r)
    assert got.report["round_trips"] == 0
    return got


def test_tie_takes_the_largest_j(host):
    check(host, tm.line_scene([(0, 10)], [(0, 13), (0, 7), (0, 20)]), [1], [0], 1, best=[3])
    check(host, tm.line_scene([(0, 10)], [(0, 7), (0, 20), (0, 13)]), [2], [0], 1, best=[3])


def test_distance_50_is_in_and_51_is_out(host):
    check(host, tm.line_scene([(0, 0), (1, 0)], [(0, 51), (1, 50)], th=100), [-1, 1], [2, 0], 1, best=[255, 50])


def test_best_equal_to_th_is_rejected(host):
    check(host, tm.line_scene([(0, 0), (1, 0)], [(0, 20), (1, 19)], th=20), [-1, 1], [2, 0], 1, best=[255, 19])


def test_candidate_that_fails_only_the_epipolar_test(host):
    # keypoint 0 is closer but on another line: it neither wins nor lowers bestDist below keypoint 1's distance
    check(host, tm.line_scene([(0, 0)], [(1, 1), (0, 9)]), [1], [0], 1, best=[9])
    check(host, tm.line_scene([(0, 0)], [(1, 1)]), [-1], [2], 0)


def test_occupied_slots_on_either_side(host):
    s = tm.line_scene([(0, 0, True), (0, 0)], [(0, 1, True), (0, 6)])
    check(host, s, [-1, 1], [1, 0], 1, best=[255, 6])


def test_more_keypoints_in_frame_2(host):
    s = tm.line_scene([(0, 0), (1, 0)], [(2, 0), (2, 1), (2, 2), (1, 5), (0, 4)])
    check(host, s, [4, 3], [0, 0], 2, best=[4, 5])


def test_steal_chain(host):
    got = check(host, tm.line_scene([(0, 30), (0, 20), (0, 13)], [(0, 10)]), [-1, -1, 0], [3, 3, 0], 1, best=[20, 10, 3])
    assert got.report["n_stolen"] == 2


def test_reverse_chain(host):
    # row 1 falls to its second choice, row 2 finds both keypoints held at distances not above its own
    s = tm.line_scene([(0, 13), (0, 20), (0, 0)], [(0, 10), (0, 40)])
    check(host, s, [0, 1, -1], [0, 0, 2], 2, best=[3, 20, 255])


def test_flag_quirk(host):
    k = 5
    s = tm.quirk_scene(2, k)
    got = check(host, s, [0] + [-1] * k, [0] + [4] * k, 1, flag_quirk=True)
    assert got.report["flag_row"] == 0 and got.report["n_flag_skipped"] == k
    got = check(host, s, np.arange(k + 1), [0] * (k + 1), k + 1, flag_quirk=False)
    assert got.report["flag_row"] == 0 and got.report["n_flag_skipped"] == 0      # the row is named in either mode
    for quirk in (True, False):                                                    # the control: distance 3
        got = check(host, tm.quirk_scene(3, k), np.arange(k + 1), [0] * (k + 1), k + 1, flag_quirk=quirk)
        assert got.report["flag_row"] == -1


@pytest.mark.parametrize("decreasing", [True, False])
def test_ten_row_chains_in_any_order(host, decreasing):
    for order in (None, np.random.default_rng(4).permutation(10)):
        s = tm.chain_scene(decreasing, order)
        r = tm.ref(s)
        assert r["n_matches"] == 2 and (r["status"] != 1).all()                   # the two keypoints end up held
        same(host.search_for_triangulation(*tm.args(s)), r)
    r = tm.ref(tm.chain_scene(decreasing))
    assert r["report"]["n_stolen"] == 8
    np.testing.assert_array_equal(r["matches"], ([1] if decreasing else [0]) + [-1] * 8 + ([0] if decreasing else [1]))


def test_cloud_scene_both_quirk_modes(host):
    s = tm.cloud_scene(65, 63, seed=1)
    for quirk in (True, False):
        r = tm.ref(s, quirk)
        same(host.search_for_triangulation(*tm.args(s, quirk)), r)
        r64 = tm.ref(s, quirk, np.float64)
        np.testing.assert_array_equal(r["matches"], r64["matches"])
    free = ~s["has1"] & (s["true2"] >= 0) & ~s["has2"][np.maximum(s["true2"], 0)]
    np.testing.assert_array_equal(r["matches"][free], s["true2"][free])            # quirk off: every planted pair


def test_th_above_255_and_null_arguments(host):
    s = tm.line_scene([(0, 0)], [(0, 3)], th=256)
    with pytest.raises(capi.DeftriError) as e:
        host.search_for_triangulation(*tm.args(s))
    assert e.value.code == _abi.DEFTRI_E_ARG and "255" in str(e.value)
    with pytest.raises(ValueError):
        tm.ref(s)
    lib = capi.load()
    n = C.c_int32(0)
    assert lib.deftri_search_for_triangulation(host.h, -1, None, None, None, 0, None, None, None, None, None, 50, 0.01, 1, None, None,
                                               None, C.byref(n), None) == _abi.DEFTRI_E_ARG
    k = np.zeros(8, np.float32)
    assert lib.deftri_search_for_triangulation(host.h, 0, None, None, None, 0, None, None, None, capi._fp(k), None, 50, 0.01, 1, None,
                                               None, None, C.byref(n), None) == _abi.DEFTRI_E_ARG


def test_empty_inputs(host):
    s = tm.line_scene([(0, 0), (0, 1, True)], [])
    got = host.search_for_triangulation(*tm.args(s))
    np.testing.assert_array_equal(got.matches, [-1, -1])
    np.testing.assert_array_equal(got.status, [2, 1])
    assert got.n_matches == 0
    same(got, tm.ref(s))
    got = host.search_for_triangulation(*tm.args(tm.line_scene([], [(0, 0)])))
    assert len(got.matches) == 0 and got.n_matches == 0


def test_report_struct_size():
    lib = capi.load()
    assert lib.deftri_sizeof(23) == C.sizeof(_abi.TriangulationMatchReport)
    assert [lib.deftri_sizeof(k) for k in (13, 19, 21)] == [-1, -1, -1] and lib.deftri_abi_version() == 8


# ---- Map.fuse_map_points / remove_map_point ------------------------------------------------------------------
def test_remove_map_point():
    m = tm.three_keyframe_map()
    m.remove_map_point(11)
    assert 11 not in m.map_points and 11 not in m.mp_obs
    assert [kf.map_points[s] for kf, s in ((m.keyframes[1], 2), (m.keyframes[2], 3), (m.keyframes[0], 4))] == [None] * 3
    assert m.kf_obs == {0: {10: 0}, 1: {10: 1}, 2: {12: 5}}
    tm.check_map(m)
    assert tm.recount_covisibility(m) == {0: {1: 1}, 1: {0: 1}}


def test_fuse_keeps_the_point_with_more_observations():
    m = tm.three_keyframe_map()
    assert m.fuse_map_points(10, 11) == 11                  # A has 2 observations, B 3: B stays, whichever comes first
    m2 = tm.three_keyframe_map()
    assert m2.fuse_map_points(11, 10) == 11                 # strictly more: mp1 is kept
    for mm in (m, m2):
        # kf0 and kf1 saw both: A's slots there are only cleared, B keeps its own
        assert 10 not in mm.map_points and mm.mp_obs[11] == {1: 2, 2: 3, 0: 4}
        assert mm.keyframes[0].map_points[0] is None and mm.keyframes[1].map_points[1] is None
        tm.check_map(mm)


def test_fuse_keeps_mp2_on_equal_counts_and_moves_observations():
    m = tm.three_keyframe_map()
    m.remove_observation(0, 11); m.keyframes[0].map_points[4] = None            # B: kf1, kf2; A: kf0, kf1
    assert m.fuse_map_points(10, 11) == 11                  # 2 against 2: mp2
    assert m.mp_obs[11] == {1: 2, 2: 3, 0: 0}               # A's observation in kf0 moved, with its slot
    assert m.keyframes[0].map_points[0] is m.map_points[11] and m.keyframes[1].map_points[1] is None
    tm.check_map(m)
    m = tm.three_keyframe_map()
    assert m.fuse_map_points(12, 10) == 10 and m.mp_obs[10] == {0: 0, 1: 1, 2: 5}   # C's only observation joins A
    assert m.keyframes[2].map_points[5] is m.map_points[10] and 12 not in m.map_points
    tm.check_map(m)
    assert m.covis[2][0] == 2 and m.covis[0][2] == 2        # kf2 now shares A and B with kf0


# ---- matching.fuse on the host-only context -------------------------------------------------------------------
def fuse_map(n=12):
    """four_views' keyframes (n + 4 keypoints each) with map points 100 .. 100 + n - 1 at the true world points of
    keypoints 0 .. n - 1, observed from keyframe 0 (slot j) only."""
    m, world = tm.four_views(n + 4)
    for j in range(n):
        mp = MapPoint(world[j].astype(np.float32), pid=100 + j)
        m.insert_map_point(mp)
        tm.observe(m, 0, mp, j)
    return m, world


def test_fuse_add_branch(host):
    n = 12
    m, _ = fuse_map(n)
    grid = dict(ps.GRID)
    m.update_orientation_and_descriptor(host, grid=grid)
    pts = [m.map_points[100 + j] for j in range(n)]
    kf = m.keyframes[2]
    n_fused, rep = matching.fuse(host, m, kf, 50, pts + [None], grid)
    assert n_fused == n and rep["n_fused"] == n and rep["rounds"] == 1 and rep["round_trips"] == 0
    for j in range(n):
        assert kf.map_points[j] is pts[j] and m.mp_obs[100 + j] == {0: j, 2: j}
    tm.check_map(m)
    assert m.covis[0][2] == n
    # a second call finds every point already in the keyframe
    assert matching.fuse(host, m, kf, 50, pts, grid)[0] == 0
    with pytest.raises(ValueError):
        matching.fuse(host, m, kf, 50, pts * 2, grid)


def test_fuse_fuse_branch_deleted_point_and_duplicate(host):
    n = 12
    m, world = fuse_map(n)
    grid = dict(ps.GRID)
    kf = m.keyframes[2]
    # keyframe 2 already holds its own points 200 + j in slots 0 .. 3: 200 and 201 are also seen from keyframe 3
    # (two observations against one: they stay), 202 and 203 from keyframe 2 alone (one against one: mp2, they stay)
    for j in range(4):
        mp = MapPoint(world[j].astype(np.float32), pid=200 + j)
        m.insert_map_point(mp)
        tm.observe(m, 2, mp, j)
        if j < 2:
            tm.observe(m, 3, mp, j)
    m.update_orientation_and_descriptor(host, grid=grid)
    pts = [m.map_points[100 + j] for j in range(n)]
    # the list: point 0 twice (the second is gone by then), point 1, a point that an earlier fusion deletes is
    # skipped at that moment, a null, and the rest
    order = [pts[0], pts[0], pts[1], None, pts[2], pts[3]] + pts[4:]
    n_fused, rep = matching.fuse(host, m, kf, 50, order, grid)
    assert n_fused == n
    for j in range(4):                                       # fused: the keyframe's own point took the observation
        assert 100 + j not in m.map_points and kf.map_points[j] is m.map_points[200 + j]
        assert m.mp_obs[200 + j][0] == j and m.keyframes[0].map_points[j] is m.map_points[200 + j]
    for j in range(4, n):                                    # added; the list index 4 + 2 reads keypoint j + 2's octave
        assert kf.map_points[j] is pts[j] and m.mp_obs[100 + j] == {0: j, 2: j}
    tm.check_map(m)
    assert len(m.map_points) == n                            # 12 + 4 - 4
    for mp in m.map_points.values():                         # one update at the end, over the surviving touched points
        assert mp.descriptor is not None and any((mp.descriptor == m.keyframes[k].descriptors[s]).all()
                                                 for k, s in m.mp_obs[mp.id].items())


def test_fuse_search_against_the_restatement(host):
    for n in (1, 65):
        s = tm.fuse_scene(n, seed=n)
        r64 = tm.fuse_ref(s, np.float64)
        assert len(s["pos"]) == n and tm.fuse_margins_ok(s, r64)
        got = host.fuse_search(*tm.fuse_args(s))
        for k in ("match", "status", "best", "second"):
            np.testing.assert_array_equal(getattr(got, k), r64[k], err_msg=k)
        assert got.report["rounds"] == 1 and got.report["n_matches"] == r64["report"]["n_matches"]
        assert float(np.abs(got.uv - r64["uv"])[s["consider"]].max(initial=0.0)) < 0.005
    bad = dict(s, octave=np.where(np.arange(n) == np.nonzero(s["consider"])[0][0], 8, s["octave"]).astype(np.int32))
    with pytest.raises(capi.DeftriError) as e:
        host.fuse_search(*tm.fuse_args(bad))
    assert e.value.code == _abi.DEFTRI_E_ARG
