"""guidedMatching, searchWithProjection (k_prepare_points, k_match_round and the claim rounds) and
Map::updateOrientationAndDescriptor (k_map_point_descriptors) on the device, against the library's sequential
host loops and the fp64 restatements of deftri.matching, and the chain map-point descriptors -> guided matching
-> poseOnlyOptimization end to end.

Matches, statuses, octaves, distances, slots and counters are integers: equal, on scenes whose fp64 restatement
decides nothing within 0.01 px of a window edge or cell boundary nor within rel 1e-3 of a threshold
(projection_scenes.margins_ok).  The projections are held to 0.005 px of the fp64 restatement, half that margin:
float resolves 1.2e-4 px at 1440 and the projection is a handful of operations.  Normals and invariance distances
are held to rel 1e-4 of the fp64 restatement, the band of this fp32 arithmetic elsewhere in the suite."""
import numpy as np
import pytest

from deftri import ba, capi, matching
from deftri.mapmodel import KeyFrame, Map, MapPoint, SE3f, mat_from_quat
from deftri.sim import inv_sigma2_table
import matching_scenes as ms
import projection_scenes as ps
import triangulation_scene as ts

gpu = pytest.mark.gpu
INT_KEYS = ("match", "status", "predicted_octave", "best", "second", "slot_point")
COUNTERS = ("n_points", "n_matches", "n_view_cos", "n_inv_dist", "n_no_candidates", "n_rejected", "n_undefined")


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


def same(got, want, ref64=None):
    for k in INT_KEYS:
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=k)
        if ref64 is not None:
            np.testing.assert_array_equal(getattr(got, k), ref64[k], err_msg=k + " (fp64)")
    for k in COUNTERS:
        assert got.report[k] == want.report[k], k
        assert ref64 is None or got.report[k] == ref64["report"][k], k


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_margin_scenes(gpu_ctx, host, n):
    s = ps.margin_scene(n, seed=n)
    r64 = ps.ref(s, np.float64)
    assert len(s["pos"]) == n and ps.margins_ok(s, r64)                    # the builder kept every case
    got, want = gpu_ctx.search_with_projection(*ps.args(s)), host.search_with_projection(*ps.args(s))
    err = float(np.abs(got.uv - r64["uv"]).max())
    print(f"n {n}: status counts {np.bincount(got.status, minlength=6)}, rounds {got.report['rounds']}, "
          f"round trips {got.report['round_trips']}, max |uv - uv64| {err:.3g} px")
    same(got, want, r64)
    assert err < 0.005
    assert 1 <= got.report["rounds"] <= n + 1 and got.report["round_trips"] == got.report["rounds"] + 1
    if n >= 63:
        assert all(got.report[k] > 0 for k in COUNTERS)                     # every branch is in the scene


@gpu
def test_more_than_64_candidates(gpu_ctx, host):
    s = ps.crowded_scene()
    r = ps.ref(s, np.float64)
    cand = matching.features_in_area(s["grid"], matching.build_grid(s["grid"], s["uv2"]), s["uv2"], s["octave2"], r["uv"][0, 0],
                                     r["uv"][0, 1], r["radius"][0], 6, 8)
    assert len(cand) > 64
    got = gpu_ctx.search_with_projection(*ps.args(s))
    same(got, host.search_with_projection(*ps.args(s)), r)
    np.testing.assert_array_equal(got.match, [70, 80, 90])


@gpu
@pytest.mark.parametrize("order", [None, "permuted"])
def test_contention_chain(gpu_ctx, host, order):
    n = 10
    perm = None if order is None else np.random.default_rng(4).permutation(n)
    s = ps.chain_scene(n, perm)
    r = ps.ref(s)
    assert (r["status"] == matching.MATCHED).all() and len(s["expect"]) >= 8   # every link passes the ratio test
    np.testing.assert_array_equal(r["match"], s["expect"])
    got, want = gpu_ctx.search_with_projection(*ps.args(s)), host.search_with_projection(*ps.args(s))
    print(order, "rounds", got.report["rounds"], got.match)
    same(got, want, r)
    assert 2 <= got.report["rounds"] <= n + 1
    assert (s["slot_point"] == -2).sum() == 2 and (got.slot_point[s["slot_point"] == -2] == -2).all()


@gpu
def test_guided_contention(gpu_ctx, host):
    """The same chain through guidedMatching: reference slots 1, 3, 5, ... hold the points."""
    s = ps.chain_scene(10, occupied=())
    n1 = 2 * len(s["pos"])
    has = np.arange(n1) % 2 == 1
    rep = lambda a: np.repeat(a, 2, axis=0)
    a = (s["grid"], s["Tcw"], s["kb8"], s["uv2"], s["octave2"], s["desc2"], has, rep(s["pos"]), np.full(n1, 2), rep(s["desc"]),
         s["th"], 1)
    got, want, r = gpu_ctx.guided_matching(*a), host.guided_matching(*a), matching.guided_matching_ref(*a)
    for k in ("match", "status", "best", "second", "slot_point"):
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=k)
        np.testing.assert_array_equal(getattr(got, k), r[k], err_msg=k)
    assert got.report["n_matches"] == 10 and 2 <= got.report["rounds"] <= n1 + 1
    assert (got.status[~has] == matching.EMPTY_SLOT).all()


@gpu
def test_map_point_descriptors(gpu_ctx, host):
    d = ps.descriptor_scene(300)
    assert set(np.diff(d["obs_start"])) == set(range(2, 10))
    got, want = gpu_ctx.map_point_descriptors(*ps.descriptor_args(d)), host.map_point_descriptors(*ps.descriptor_args(d))
    r64 = matching.map_point_descriptors_ref(*ps.descriptor_args(d), dtype=np.float64)
    for k in ("desc", "ref_obs", "status"):
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=k)
        np.testing.assert_array_equal(getattr(got, k), r64[k], err_msg=k)
    assert len(set(got.ref_obs)) >= 6
    e_n = float(np.abs(got.normal - r64["normal"]).max())
    e_mx, e_mn = float(np.abs(got.max_dist / r64["max_dist"] - 1).max()), float(np.abs(got.min_dist / r64["min_dist"] - 1).max())
    print(f"max errors against fp64: normal {e_n:.3g}, max_dist rel {e_mx:.3g}, min_dist rel {e_mn:.3g}")
    assert e_n < 1e-4 and e_mx < 1e-4 and e_mn < 1e-4


def chain_map(n=200, n_outliers=10):
    """triangulation_scene's two views as a two-keyframe map with synthetic descriptors, and a third frame seen from
    between them: keypoint j of every frame belongs to map point j.  The frame's first n_outliers keypoints are
    moved by 8 px: still matched by descriptor, outliers for the pose."""
    rng = np.random.default_rng(7)
    uv1, uv2, k1, k2, T1w, T2w, info = ts.scene(n, seed=2, offsets=False, nans=0)
    inv = inv_sigma2_table(ps.N_SCALES, ps.FACTOR)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    noisy = lambda: np.stack([ms.flip_bits(d, rng.choice(256, rng.integers(0, 8), replace=False)) for d in desc])
    kf1 = KeyFrame(0, T1w, k1, n, inv, keypoints=uv1, octaves=np.zeros(n, np.int32), descriptors=noisy())
    kf2 = KeyFrame(1, T2w, k2, n, inv, keypoints=uv2, octaves=np.zeros(n, np.int32), descriptors=noisy())
    m = Map()
    m.insert_keyframe(kf1); m.insert_keyframe(kf2)
    for j in range(n):
        mp = MapPoint(info["world"][j].astype(np.float32), pid=j)
        m.insert_map_point(mp)
        kf1.map_points[j] = kf2.map_points[j] = mp
        m.add_observation(0, j, j); m.add_observation(1, j, j)
    q = np.array([0.001, 0.004, 0.003, 1.0]); q /= np.linalg.norm(q)
    R = mat_from_quat(q).astype(np.float32)
    c = np.array([0.03, 0.002, -0.015], np.float32)
    true_pose = SE3f(R, -(R @ c))
    world = info["world"]
    uv = ts._project64(k1, world @ R.astype(np.float64).T + true_pose.t.astype(np.float64)) + rng.normal(0, 0.1, (n, 2))
    uv[:n_outliers, 0] += 8.0
    q2 = np.array([0.001 + 0.002, 0.004 - 0.002, 0.003 + 0.001, 1.0]); q2 /= np.linalg.norm(q2)
    R2 = mat_from_quat(q2).astype(np.float32)
    start = SE3f(R2, -(R2 @ (c + np.array([0.002, -0.001, 0.001], np.float32))))
    frame = KeyFrame(2, start, k1, n, inv, keypoints=uv.astype(np.float32), octaves=np.zeros(n, np.int32), descriptors=noisy())
    return m, kf1, frame, true_pose


def pose_distance(a, b):
    d = a * b.inverse()
    return float(np.linalg.norm(d.t)) + float(np.arccos(np.clip((np.trace(d.R.astype(np.float64)) - 1) / 2, -1, 1)))


@gpu
def test_chain_to_pose_only_optimization(gpu_ctx):
    n, n_outliers = 200, 10
    m, kf1, frame, true_pose = chain_map(n, n_outliers)
    grid = dict(ps.GRID)
    status = m.update_orientation_and_descriptor(gpu_ctx, grid=grid)
    assert (status == 0).all() and all(mp.descriptor is not None for mp in m.map_points.values())
    matches, report = matching.guided_matching(gpu_ctx, kf1, frame, grid, 50, 1)
    n_matches = report["n_matches"]
    print("matches", n_matches, "rounds", report["rounds"], "statuses", np.bincount(np.asarray(matches) >= 0))
    assert n_matches >= 0.9 * n
    for j, mp in enumerate(frame.map_points):                              # the matched slots hold the right map points
        assert mp is None or mp.id == j
    np.testing.assert_array_equal(matches[matches >= 0], np.nonzero(matches >= 0)[0])
    planted = sum(frame.map_points[j] is not None for j in range(n_outliers))
    before = pose_distance(frame.pose, true_pose)
    n_good = ba.poseOnlyOptimization(frame)
    after = pose_distance(frame.pose, true_pose)
    print("inliers", n_good, "planted outliers matched", planted, "pose distance", before, "->", after)
    assert n_good == n_matches - planted
    assert after < before
