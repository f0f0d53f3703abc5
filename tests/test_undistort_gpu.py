"""deftri_undistort_points and deftri_distribute_features on the device (k_undistort, k_undistort_cells, then the
matchers' k_excl_scan / k_grid_fill and k_grid_order) against the library's sequential host loops and
undistort_ref.py, every output array bit for bit: both sides evaluate the same double operations with one rounding
each, posInGrid in float, and the cell lists are integers in keypoint order.

The sizes 0, 1, 63, 64, 65 and 257 cover one lane, the wave boundary, the 256-thread block boundary and a ragged
tail: the smallest at which the tail guard, the per-lane early break and the order within a cell can go wrong.
Then the Python chain end to end: an image through extract_features with its third line, and two keyframes through
monocular_map_initialization_from_features under Camera.k1 settings."""
import numpy as np
import pytest

from deftri import capi, features, mapping, matching, sim
from deftri.mapmodel import KeyFrame
from deftri.settings import Settings
import features_ref as fr
import triangulation_scene as ts
import undistort_ref as ur
from test_matching_gpu import _pair, _reset, _snapshot, settings_text
from test_orb import PATTERN

gpu = pytest.mark.gpu
F = np.float32
NEGATIVE_ICDIST = np.array([-2, 0, 0, 0], F)


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


def _point_sets():
    uv = ur.points()
    nan = np.array([[np.nan, 100.0], [100.0, np.nan], [300.0, 200.0]], F)
    # k1 = -2: the lanes at normalized radius 1 and beyond stop in their first iteration, the others go on
    ring = np.array([[ur.CALIB[2] + ur.CALIB[0], ur.CALIB[3]], [400.0, 250.0], [ur.CALIB[2], ur.CALIB[3] - ur.CALIB[1]]], F)
    return {"k1k2p1p2": (uv, ur.DIST4), "k3": (uv, ur.DIST5), "zeros": (uv, np.zeros(4, F)), "nan": (nan, ur.DIST4),
            "negative_icdist": (np.concatenate([ring, uv]), NEGATIVE_ICDIST)}


@gpu
@pytest.mark.parametrize("name", sorted(_point_sets()))
def test_points_on_device(gpu_ctx, host, name):
    uv, dist = _point_sets()[name]
    got = ur.check_points(gpu_ctx, uv, ur.CALIB, dist)
    ur.same_bits(got, host.undistort_points(uv, ur.CALIB, dist))
    if name == "negative_icdist":
        stopped = np.array([1 / (1 + float(dist[0]) * r2) < 0 for r2 in (((uv.astype(np.float64) - ur.CALIB[2:]) / ur.CALIB[:2]) ** 2).sum(1)])
        assert stopped[0] and not stopped[1] and 0 < stopped.sum() < len(uv)
    assert gpu_ctx.undistort_points(uv[:0], ur.CALIB, dist).shape == (0, 2)


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_points_tail_on_device(gpu_ctx, n):
    """A point is one thread's work: the first n of the set equal rows [:n] of the whole."""
    uv = ur.points()
    ur.same_bits(gpu_ctx.undistort_points(uv[:n], ur.CALIB, ur.DIST4), ur.undistort(uv, ur.CALIB, ur.DIST4)[:n])


@gpu
@pytest.mark.parametrize("n", ur.SIZES)
@pytest.mark.parametrize("dist", [ur.DIST4, ur.DIST5, np.zeros(0, F)], ids=["k1k2p1p2", "k3", "none"])
def test_distribute_on_device(gpu_ctx, host, n, dist):
    uv_dis = ur.grid_keys(n)
    want = ur.distribute(uv_dis, ur.CALIB, dist)
    got = ur.check_distribute(gpu_ctx, uv_dis, ur.CALIB, dist, want)
    hst = ur.check_distribute(host, uv_dis, ur.CALIB, dist, want)
    ur.same_bits(got.uv, hst.uv)
    assert got.grid == hst.grid and got.cell_start.tobytes() == hst.cell_start.tobytes()
    assert got.cell_items.tobytes() == hst.cell_items.tobytes() and got.in_grid.tobytes() == hst.in_grid.tobytes()
    if n >= 63 and len(dist):
        assert max(np.diff(got.cell_start)) >= 2 and got.in_grid[n - 4:].tolist() == [False, False, False, True]


@gpu
def test_crowded_cell_keeps_keypoint_order(gpu_ctx, host):
    """300 zero slots behind 65 keypoints, as a frame of nFeatures slots has: they all undistort to one position and
    share one cell, whose list the device must still hold in keypoint order."""
    uv_dis = np.concatenate([ur.grid_keys(65), np.zeros((300, 2), F)])
    got = ur.check_distribute(gpu_ctx, uv_dis, ur.CALIB, ur.DIST4)
    assert got.cells()[0][0][-300:] == list(range(65, 365))


def _image_settings(distorted):
    """The Simulation calibration scaled to a 160 x 120 image, with or without its distortion keys."""
    sx, sy = 160 / ur.COLS, 120 / ur.ROWS
    cam = f"Camera.fx: {ur.CALIB[0] * sx}\nCamera.fy: {ur.CALIB[1] * sy}\nCamera.cx: {ur.CALIB[2] * sx}\nCamera.cy: {ur.CALIB[3] * sy}\n"
    k = "".join(f"Camera.{name}: {float(v)!r}\n" for name, v in zip(("k1", "k2", "p1", "p2"), ur.DIST4.astype(np.float64)))
    return Settings(text=cam + (k if distorted else "") + "Camera.cols: 160\nCamera.rows: 120\nFeatureGrid.nGridCols: 16\n"
                    "FeatureGrid.nGridRows: 12\nFeatureExtractor.nScales: 2\nFeatureExtractor.fScaleFactor: 1.2\n"
                    "FeatureExtractor.nFeatures: 300\n")


@gpu
def test_image_to_undistorted_keyframe(gpu_ctx):
    image, _ = fr.make_scene(120, 160, 1)
    s, plain = _image_settings(True), _image_settings(False)
    assert s.distortion.tobytes() == ur.DIST4.tobytes() and not plain.has_distortion
    keys, desc, dist = mapping.extract_features(gpu_ctx, image, s, PATTERN, distribute=True, n_slots=300)
    n = len(keys)
    assert 20 < n < 300 and len(dist) == 300 and len(mapping.extract_features(gpu_ctx, image, s, PATTERN)) == 2
    kf = KeyFrame(0, ts.poses()[0], ts.KB8_1, 300, sim.inv_sigma2_table(2, 1.2))
    assert kf.keypoints_dis is None
    assert mapping.set_keypoints_from_features(kf, keys, desc, dist) == n
    calib = np.array([s.fx, s.fy, s.cx, s.cy], F)
    slots = np.concatenate([keys.uv, np.zeros((300 - n, 2), F)])
    want = ur.distribute(slots, calib, ur.DIST4, 160, 120, n_scales=2)
    ur.same_bits(kf.keypoints, want[0])                       # vKeys_: undistorted, the zero slots behind them too
    ur.same_bits(kf.keypoints[:n], ur.undistort(keys.uv, calib, ur.DIST4))
    ur.same_bits(kf.keypoints_dis, slots)                     # vKeysDis_: what FAST found
    assert np.abs(kf.keypoints[:n] - keys.uv).max() > 0.5
    assert dist.grid == dict(want[1], scale_factor=dist.grid["scale_factor"]) == matching.frame_grid(gpu_ctx, s) | {
        "scale_factor": dist.grid["scale_factor"]}
    assert dist.cell_start.tolist() == want[2].tolist() and dist.cell_items.tolist() == want[3].tolist()
    # FAST and ORB read the distorted image and keys: the same as without Camera.k1, bit for bit
    keys0, desc0 = mapping.extract_features(gpu_ctx, image, plain, PATTERN)
    assert keys0.uv.tobytes() == keys.uv.tobytes() and keys0.octave.tobytes() == keys.octave.tobytes()
    assert desc0.desc.tobytes() == desc.desc.tobytes() and kf.descriptors[:n].tobytes() == desc.desc.tobytes()
    # without Camera.k1 the third line copies the keys
    _, _, same = mapping.extract_and_distribute_features(gpu_ctx, image, plain, PATTERN)
    assert same.uv.tobytes() == keys.uv.tobytes() and same.grid["max_col"] == 160 and same.grid["min_col"] == 0


SMALL_CAMERA = "\nCamera.fx: 70.0\nCamera.fy: 70.0\nCamera.cx: 32.0\nCamera.cy: 32.0\n"      # triangulation_scene.KB8_SMALL_1's pinhole part


@gpu
def test_two_keyframes_under_distortion(gpu_ctx, host):
    """Two keyframes whose keys are given as distorted pixels: the map from monocular_map_initialization_from_features
    under Camera.k1 settings equals the one the no-distortion path builds when it is fed by hand with the
    reference-undistorted keys and the frame_grid bounds: nothing between the grid and the map reads the settings
    again."""
    kf_ref, kf_cur, perm = _pair()
    plain = Settings(text=settings_text() + SMALL_CAMERA)
    k = "".join(f"Camera.{name}: {float(v)!r}\n" for name, v in zip(("k1", "k2", "p1", "p2"), ur.DIST4.astype(np.float64)))
    st = Settings(text=settings_text() + SMALL_CAMERA + k)
    assert st.has_distortion and not plain.has_distortion
    calib = np.array([70, 70, 32, 32], F)
    dis = [ur.distort(kf.keypoints, calib, ur.DIST4) for kf in (kf_ref, kf_cur)]       # the distorted pixels of the scene's keys
    und = [ur.undistort(d, calib, ur.DIST4) for d in dis]
    assert all(np.abs(u - kf.keypoints).max() < 0.05 < np.abs(d - kf.keypoints).max() for u, d, kf in zip(und, dis, (kf_ref, kf_cur)))
    grid = matching.frame_grid(gpu_ctx, st)
    assert grid == dict(ur.grid_of(ur.image_bounds(64, 64, calib, ur.DIST4), 8, 8, 8, 1.2), scale_factor=1.2)
    assert grid["min_col"] < 0 and grid["min_row"] < 0
    try:
        # by hand: the reference's undistorted keys, the existing matcher on that grid, the existing initialization
        for kf, u in zip((kf_ref, kf_cur), und):
            kf.keypoints = u.copy()
        hm, _, _, hn = host.match_for_initialization(grid, kf_ref.keypoints, kf_ref.octaves, kf_ref.descriptors, kf_cur.keypoints,
                                                     kf_cur.octaves, kf_cur.descriptors, plain.matching_init_th,
                                                     plain.matching_init_radius)
        assert hn >= 100
        _reset(kf_ref, kf_cur)
        m1, rep1 = mapping.monocular_map_initialization(gpu_ctx, kf_ref, kf_cur, hm.astype(np.int64), plain)
        assert m1 is not None and rep1["accepted"] == 1 and rep1["n_map_points"] > 50
        want = _snapshot(m1, kf_ref, kf_cur)
        # the library's chain: distorted keys into the keyframes through distribute, then the Camera.k1 settings
        _reset(kf_ref, kf_cur)
        for kf, d in zip((kf_ref, kf_cur), dis):
            res = capi.FastResult(d, kf.octaves.copy(), np.zeros(len(d), F), np.zeros(len(d), F), np.zeros(len(d), F), {})
            mapping.set_keypoints_from_features(kf, res, None, features.distribute(gpu_ctx, res, st))
            assert kf.keypoints_dis.tobytes() == d.tobytes()
        ur.same_bits(kf_ref.keypoints, und[0]); ur.same_bits(kf_cur.keypoints, und[1])
        m2, rep2 = mapping.monocular_map_initialization_from_features(gpu_ctx, kf_ref, kf_cur, st)
        assert m2 is not None and _snapshot(m2, kf_ref, kf_cur) == want
        assert rep2["n_matches"] == hn and {k_: v for k_, v in rep2.items() if k_ in rep1} == rep1
    finally:
        gpu_ctx.set_depth_images([])
