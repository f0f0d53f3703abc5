"""searchForInitializaion (k_match_init over the device's cell lists) and the epipolar inlier mask
(k_epipolar_inliers) on the device, against the library's sequential host loops and the numpy restatements
of deftri.matching, and mapping.monocular_map_initialization_from_features end to end.

Matches, distances, counts and the cell lists are integers: equal.  The epipolar error is held to 2e-6
absolute against the fp64 restatement: float resolves 1.2e-7 at pi/2, the dot of two unit vectors near 0
carries a few 1e-7 and acos is well conditioned there (cos_parallax is held to 1e-6 in the same family).
Flags and score equal the fp32 restatement's on a scene whose fp64 errors all lie further than rel 1e-3 from
the threshold (the margins_ok convention of triangulation_scene)."""
import numpy as np
import pytest

from conftest import GOLDEN
from deftri import capi, mapping, matching, sim
from deftri.mapmodel import KeyFrame, Map
from deftri.settings import Settings
import depth_image_ref as ref
import matching_scenes as ms
import triangulation_scene as ts

gpu = pytest.mark.gpu
EPI_TH = 0.035          # splits triangulation_scene's correspondences (asserted below with the fp64 restatement)


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


def _same(got, want):
    for g, w in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(g, w)
    assert got[3] == want[3]


SCENES = {"n64": lambda: ms.random_scene(64, ms.SMALL, 15.0, seed=1), "n257": lambda: ms.random_scene(257, ms.SMALL, 15.0, seed=2),
          "realcolon2048": lambda: ms.random_scene(2048, ms.REALCOLON, 25.0, seed=3), "crowded": lambda: ms.window_scene(300, seed=4),
          "window64": lambda: ms.window_scene(64, 100, seed=5), "window65": lambda: ms.window_scene(65, 100, seed=6)}


@gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_equals_host_loop(gpu_ctx, host, name):
    s = SCENES[name]()
    want = host.match_for_initialization(*ms.args(s))
    got = gpu_ctx.match_for_initialization(*ms.args(s))
    print(name, got[3], int((got[0] >= 0).sum()))
    _same(got, want)
    assert got[3] == int((got[0] >= 0).sum()) >= 1
    if name.startswith("window") or name == "crowded":
        g = s["grid"]
        cand = matching.features_in_area(g, matching.build_grid(g, s["uv2"]), s["uv2"], s["octave2"], s["uv1"][0, 0], s["uv1"][0, 1],
                                         np.float32(s["radius"]), -1, 1)
        assert len(cand) == {"window64": 64, "window65": 65}.get(name, len(cand)) and (name != "crowded" or len(cand) >= 129)
        assert got[0][0] >= 0


@gpu
@pytest.mark.parametrize("name", sorted(ms.quirk_scenes()))
def test_quirk_on_device(gpu_ctx, host, name):
    s = ms.quirk_scenes()[name]
    got = gpu_ctx.match_for_initialization(*ms.args(s))
    np.testing.assert_array_equal(got[0], s["expect"])
    _same(got, host.match_for_initialization(*ms.args(s)))


@gpu
def test_acceptance_on_device(gpu_ctx, host):
    """Every (best, second) in [0, 256]^2: the device's acceptance and reduction equal the host loop's."""
    s = ms.acceptance_scene()
    got = gpu_ctx.match_for_initialization(*ms.args(s))
    _same(got, host.match_for_initialization(*ms.args(s)))
    assert np.array_equal(got[0] >= 0, 10 * got[1] < 9 * got[2])


@gpu
def test_unsearched_and_empty_on_device(gpu_ctx):
    s = ms.quirk_scenes()["two_to_one"]
    a = ms.args(s)
    m, best, second, n = gpu_ctx.match_for_initialization(a[0], a[1], a[2], a[3], s["uv2"][:0], s["octave2"][:0], s["desc2"][:0],
                                                          100, 25.0)
    assert list(m) == [-1, -1] and list(best) == [255, 255] and n == 0
    with pytest.raises(capi.DeftriError, match="octave"):
        gpu_ctx.match_for_initialization(a[0], a[1], np.array([0, 8], np.int32), *a[3:])


@gpu
@pytest.mark.parametrize("n,cells", [
    pytest.param(1, None, id="1"), pytest.param(257, None, id="257"), pytest.param(2048, None, id="2048"),
    # the scan's chunk boundaries: 1, 255, 256, 257 and 1000 cells against the 256 threads of its one workgroup
    pytest.param(300, (1, 1), id="300-1cell"), pytest.param(300, (15, 17), id="300-255cells"),
    pytest.param(300, (16, 16), id="300-256cells"), pytest.param(300, (257, 1), id="300-257cells"),
    pytest.param(300, (40, 25), id="300-1000cells")])
def test_cell_lists(gpu_ctx, host, n, cells):
    """Every in-grid key exactly once, in its own cell; out-of-grid keys nowhere."""
    grid = ms.REALCOLON if cells is None else dict(ms.REALCOLON, cols=cells[0], rows=cells[1])
    s = ms.random_scene(n, grid, 25.0, seed=8)
    g, uv = s["grid"], s["uv2"]
    uv[0] = [1429.0 if cells is None else 1439.5, 500.0]      # the last half cell: in no cell
    assert not matching.pos_in_grid(g, *uv[0])[0]
    start, keys = gpu_ctx.debug_feature_grid_cells(g, uv)
    hstart, hkeys = host.debug_feature_grid_cells(g, uv)
    np.testing.assert_array_equal(start, hstart)
    assert 0 not in keys and len(keys) == start[-1]
    for c in np.flatnonzero(np.diff(start)):                  # the same keys per cell, in any order
        assert sorted(keys[start[c]:start[c + 1]].tolist()) == hkeys[hstart[c]:hstart[c + 1]].tolist()
    inside = np.array([matching.pos_in_grid(g, x, y)[0] for x, y in uv])
    assert sorted(keys.tolist()) == np.flatnonzero(inside).tolist()


@gpu
@pytest.mark.parametrize("n", [120, 257])
def test_epipolar_inliers_on_device(gpu_ctx, n):
    uv1, uv2, k1, k2, T1w, T2w, _ = ts.scene(n, nans=0)
    inl64, err64, _ = matching.epipolar_inliers(uv1, uv2, k1, k2, T1w, T2w, EPI_TH, np.float64)
    assert (np.abs(err64 - EPI_TH) > 1e-3 * EPI_TH).all() and 0.1 * n <= inl64.sum() <= 0.9 * n
    inl32, _, score32 = matching.epipolar_inliers(uv1, uv2, k1, k2, T1w, T2w, EPI_TH, np.float32)
    inl, err, score = gpu_ctx.epipolar_inliers(uv1, uv2, k1, k2, T1w, T2w, EPI_TH)
    print(n, score, "max |err - fp64|", np.abs(err.astype(np.float64) - err64).max())
    assert np.abs(err.astype(np.float64) - err64).max() <= 2e-6
    np.testing.assert_array_equal(inl, inl32)
    assert score == score32 == int(inl.sum())
    # without a threshold to pass nothing is an inlier: the reference's empty vBestInliers
    assert gpu_ctx.epipolar_inliers(uv1, uv2, k1, k2, T1w, T2w, 0.0)[2] == 0


@gpu
@pytest.mark.parametrize("k", [8, 255, 256])
def test_epipolar_inliers_prefix_is_bit_identical(gpu_ctx, k):
    """Every match is one thread's work, independent of n: a call on the first k (8 is the entry's minimum)
    equals rows [:k] of the call on all 257, across the 256-thread block and the 256-byte padding of the
    call's device arena pieces."""
    uv1, uv2, k1, k2, T1w, T2w, _ = ts.scene(257, nans=0)
    inl, err, _ = gpu_ctx.epipolar_inliers(uv1, uv2, k1, k2, T1w, T2w, EPI_TH)
    pinl, perr, pscore = gpu_ctx.epipolar_inliers(uv1[:k], uv2[:k], k1, k2, T1w, T2w, EPI_TH)
    np.testing.assert_array_equal(pinl, inl[:k])
    np.testing.assert_array_equal(perr.view(np.uint32), err[:k].view(np.uint32))
    assert pscore == int(inl[:k].sum())


# ---- end to end: two keyframes over 64 x 64 depth images, synthetic descriptors ----
N_REAL = 200
YAML_TAIL = ("\nCamera.cols: 64\nCamera.rows: 64\nFeatureGrid.nGridCols: 8\nFeatureGrid.nGridRows: 8\n"
             "FeatureExtractor.nFeatures: 200\nFeatureExtractor.nScales: 8\nFeatureExtractor.fScaleFactor: 1.2\n"
             "Matching.initialization: 50\nMatching.initialization.radius: 40\nTriangulation.minMatches: 30\n"
             "Triangulation.depthLimit: 10.0\n")


def settings_text():
    """The simulation settings without their OpenCV distortion keys (a real-image YAML such as Realcolon's
    has none), and the front end's keys for the 64 x 64 images."""
    base = (GOLDEN / "sim_default" / "settings.yaml").read_text().splitlines()
    return "\n".join(ln for ln in base if not ln.startswith(("Camera.k", "Camera.p"))) + YAML_TAIL


def _pair():
    uv1, uv2, k1, k2, T1w, T2w, info = ts.scene(N_REAL, seed=1, kb8_1=ts.KB8_SMALL_1, kb8_2=ts.KB8_SMALL_2, offsets=False, nans=0)
    rng = np.random.default_rng(3)
    perm = rng.permutation(N_REAL)
    kp2 = np.zeros_like(uv2); z2 = np.zeros(N_REAL)
    kp2[perm] = uv2; z2[perm] = info["z2"]
    d1 = rng.integers(0, 256, (N_REAL, 32), dtype=np.uint8)
    d2 = np.zeros_like(d1)
    for i in range(N_REAL):
        d2[perm[i]] = ms.flip_bits(d1[i], rng.choice(256, rng.integers(0, 10), replace=False))
    inv_s2 = sim.inv_sigma2_table(8, 1.2)
    oct1 = np.where(np.arange(N_REAL) % 9 == 0, 1, 0)
    kf_ref = KeyFrame(0, T1w, k1, N_REAL, inv_s2, uv1, oct1, info["z1"], descriptors=d1)
    kf_cur = KeyFrame(1, T2w, k2, N_REAL, inv_s2, kp2, np.zeros(N_REAL, np.int32), z2, descriptors=d2)
    m = Map()
    m.insert_keyframe(kf_ref); m.insert_keyframe(kf_cur)
    ref.synthetic_images(m, (64, 64), seed=5)
    return kf_ref, kf_cur, perm


def _snapshot(m, kf_ref, kf_cur):
    slots = [[None if mp is None else (mp.id, tuple(np.asarray(mp.position).tolist())) for mp in kf.map_points]
             for kf in (kf_ref, kf_cur)]
    return {"slots": slots, "ids": sorted(m.map_points), "obs": {k: dict(v) for k, v in m.kf_obs.items()},
            "scales": (kf_ref.estimated_depth_scale, kf_cur.estimated_depth_scale)}


def _reset(kf_ref, kf_cur):
    for kf in (kf_ref, kf_cur):
        kf.map_points = [None] * N_REAL
        kf.estimated_depth_scale = 1.0


@gpu
@pytest.mark.parametrize("checks", [False, True])
def test_map_initialization_from_features(gpu_ctx, host, checks):
    kf_ref, kf_cur, perm = _pair()
    st = Settings(text=settings_text())
    st.trian_checks = checks
    grid = matching.feature_grid(st)
    # the host loop's matches (and mask): what monocular_map_initialization is fed with
    hm, _, _, hn = host.match_for_initialization(grid, kf_ref.keypoints, kf_ref.octaves, kf_ref.descriptors, kf_cur.keypoints,
                                                 kf_cur.octaves, kf_cur.descriptors, st.matching_init_th, st.matching_init_radius)
    idx = np.flatnonzero(hm >= 0)
    assert hn == len(idx) >= 100 and (hm[kf_ref.octaves > 0] == -1).all() and np.array_equal(hm[idx], perm[idx])
    fed = hm.astype(np.int64)
    if checks:
        p1, p2 = kf_ref.keypoints[idx], kf_cur.keypoints[hm[idx]]
        e64 = np.sort(matching.epipolar_inliers(p1, p2, kf_ref.kb8, kf_cur.kb8, kf_ref.pose, kf_cur.pose, 1.0, np.float64)[1])
        lo, hi = len(e64) // 4, 3 * len(e64) // 4                           # the widest gap of the central half
        k = lo + int(np.argmax(np.diff(e64[lo:hi])))
        st.epipolar_th = float(0.5 * (e64[k] + e64[k + 1]))
        assert (np.abs(e64 - st.epipolar_th) > 1e-3 * st.epipolar_th).all()
        hin, _, hscore = host.epipolar_inliers(p1, p2, kf_ref.kb8, kf_cur.kb8, kf_ref.pose, kf_cur.pose, st.epipolar_th)
        assert hscore == k + 1 and 0 < hscore < len(idx)
        fed[idx[~hin]] = -1
    try:
        _reset(kf_ref, kf_cur)
        m1, rep1 = mapping.monocular_map_initialization(gpu_ctx, kf_ref, kf_cur, fed, st)
        assert m1 is not None and rep1["accepted"] == 1 and rep1["n_map_points"] > 50
        want = _snapshot(m1, kf_ref, kf_cur)
        _reset(kf_ref, kf_cur)
        m2, rep2 = mapping.monocular_map_initialization_from_features(gpu_ctx, kf_ref, kf_cur, st)
        assert m2 is not None and _snapshot(m2, kf_ref, kf_cur) == want
        assert rep2["n_matches"] == hn and {k: v for k, v in rep2.items() if k in rep1} == rep1
        assert ("n_inliers" in rep2) == checks
        # too few matches (Mapping.cc:151-156)
        st.min_matches = hn + 1
        m3, rep3 = mapping.monocular_map_initialization_from_features(gpu_ctx, kf_ref, kf_cur, st)
        assert m3 is None and rep3["n_matches"] == hn and rep3["accepted"] == 0
        st.min_matches = hn
        if checks:                                            # a score of 0: nothing to triangulate
            st.epipolar_th = 0.0
            m4, rep4 = mapping.monocular_map_initialization_from_features(gpu_ctx, kf_ref, kf_cur, st)
            assert m4 is None and rep4["n_inliers"] == 0 and rep4["n_matches"] == hn
    finally:
        gpu_ctx.set_depth_images([])
