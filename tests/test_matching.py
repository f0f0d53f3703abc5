"""searchForInitializaion and the epipolar inlier mask without a GPU: the library's sequential host loops (a
host-only context) against the independent numpy restatements of deftri.matching, each quirk of the reference
with its own assertion, and the argument checks.

No golden from the reference is possible (its matcher needs OpenCV); parity is held device against host loop
(test_matching_gpu.py) against the numpy restatement (here).  Matches and distances are integers: equal.
The epipolar error is held to 2e-6 absolute between the fp32 restatement and the host loop (float resolves
1.2e-7 at pi/2, the dot of two unit vectors near 0 carries a few 1e-7, acos is well conditioned there)."""
import ctypes as C

import numpy as np
import pytest

from deftri import _abi, capi, mapping, matching
from deftri.mapmodel import KeyFrame
from deftri.settings import Settings
import matching_scenes as ms
import triangulation_scene as ts

EPI_TH = 0.035          # splits triangulation_scene's correspondences (checked in the tests below)


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def scenes():
    """The device scenes of test_matching_gpu.py with the numpy restatement's result, computed once."""
    out = {"n64": ms.random_scene(64, ms.SMALL, 15.0, seed=1), "n257": ms.random_scene(257, ms.SMALL, 15.0, seed=2),
           "realcolon2048": ms.random_scene(2048, ms.REALCOLON, 25.0, seed=3), "crowded": ms.window_scene(300, seed=4),
           "window64": ms.window_scene(64, 100, seed=5), "window65": ms.window_scene(65, 100, seed=6)}
    return {k: (s, matching.search_for_initialization(*ms.args(s))) for k, s in out.items()}


def candidates_of_first(s):
    g = s["grid"]
    cells = matching.build_grid(g, s["uv2"])
    return matching.features_in_area(g, cells, s["uv2"], s["octave2"], s["uv1"][0, 0], s["uv1"][0, 1], np.float32(s["radius"]), -1, 1)


def test_hamming_against_unpackbits():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (1000, 32), dtype=np.uint8); b = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    b[:50] = a[:50]; b[50:60] = ~a[50:60]
    want = np.unpackbits(a ^ b, axis=1).sum(1)
    assert np.array_equal(matching.hamming(a, b), want) and want[:50].max() == 0 and want[50:60].min() == 256
    assert matching.hamming(a[100], b[100]) == want[100]


def test_round_is_half_away_from_zero():
    g = dict(ms.REALCOLON)
    assert matching.pos_in_grid(g, 11.25, 11.25) == (True, 1, 1)           # 0.5 rounds to 1 (numpy.round gives 0)
    assert matching.pos_in_grid(g, 56.25, 33.75) == (True, 3, 2)           # 2.5 -> 3, 1.5 -> 2
    assert matching.pos_in_grid(g, -11.25, 0.0)[0] is False                # -0.5 -> -1
    assert matching.pos_in_grid(g, 1428.75, 0.0)[0] is False and matching.pos_in_grid(g, 1428.7, 0.0) == (True, 63, 0)
    assert matching.pos_in_grid(g, np.nan, 0.0)[0] is False


def test_acceptance_is_the_literal_double_expression(host):
    """All (best, second) in [0, 256]^2 through two-candidate scenes on the host loop."""
    s = ms.acceptance_scene()
    m, best, second, nm = host.match_for_initialization(*ms.args(s))
    b, sd = s["b"], s["s"]
    lo, hi = np.minimum(b, sd), np.maximum(b, sd)
    want_best = np.where(lo < 255, lo, 255)
    want_second = np.where(hi < 255, hi, 255)
    assert np.array_equal(best, want_best) and np.array_equal(second, want_second)
    literal = np.array([bb <= s["th"] and float(np.float32(bb)) < float(np.float32(ss)) * 0.9
                        for bb, ss in zip(want_best.tolist(), want_second.tolist())])
    assert np.array_equal(m >= 0, literal) and nm == int(literal.sum())
    assert np.array_equal(literal, 10 * want_best < 9 * want_second)       # th = 256 never binds
    n = len(b)
    want_idx = np.where(b <= sd, np.arange(n), np.arange(n) + n)            # the candidate at the smaller distance
    assert np.array_equal(m[literal], want_idx[literal])
    assert not literal[b == sd].any()                                      # a tie for best always rejects
    # the numpy restatement's acceptance is the same expression
    assert all(matching.accept(int(x), int(y), 256) == bool(z) for x, y, z in zip(want_best[::97], want_second[::97], literal[::97]))


@pytest.mark.parametrize("name", ["n64", "n257", "realcolon2048", "crowded", "window64", "window65"])
def test_host_loop_equals_numpy(host, scenes, name):
    s, want = scenes[name]
    got = host.match_for_initialization(*ms.args(s))
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert got[3] == want[3]
    if name in ("n64", "n257", "realcolon2048"):
        n1 = len(s["uv1"])
        assert 0.3 * n1 < got[3] < n1 and (got[0][s["octave1"] > 0] == -1).all()
    else:
        assert got[0][0] >= 0 and got[3] >= 1


def test_window_scenes_hold_what_they_claim(scenes):
    assert len(candidates_of_first(scenes["window64"][0])) == 64
    assert len(candidates_of_first(scenes["window65"][0])) == 65
    crowded = scenes["crowded"][0]
    assert len(crowded["uv2"]) == 300 and 129 <= len(candidates_of_first(crowded)) <= 256


@pytest.mark.parametrize("name", sorted(ms.quirk_scenes()))
def test_quirk(host, name):
    s = ms.quirk_scenes()[name]
    want = matching.search_for_initialization(*ms.args(s))
    assert np.array_equal(want[0], s["expect"]), (name, want)
    got = host.match_for_initialization(*ms.args(s))
    assert np.array_equal(got[0], s["expect"]) and got[3] == int((s["expect"] >= 0).sum())
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    if name.startswith("last_half_cell"):
        assert got[1][0] == 255 and got[1][1] == 1          # the only candidate of keypoint 0 is in no cell
    if name == "tie_for_best":
        assert got[1][0] == got[2][0] == 2
    if name == "best_equals_th":
        assert list(got[1]) == [20, 21]
    if name == "distance_256":
        assert list(got[1]) == [255, 255] and list(got[2]) == [255, 255]
    if name == "current_octave_2":
        assert got[1][0] == 255


def test_cell_lists_host(host):
    s = ms.random_scene(257, ms.REALCOLON, 25.0, seed=8)
    uv = s["uv2"]
    start, keys = host.debug_feature_grid_cells(s["grid"], uv)
    inside = np.array([matching.pos_in_grid(s["grid"], x, y)[0] for x, y in uv])
    assert 0 < (~inside).sum() and sorted(keys.tolist()) == np.flatnonzero(inside).tolist()
    assert start[0] == 0 and start[-1] == inside.sum() and (np.diff(start) >= 0).all()
    for k in (0, 5, 100):
        _, c, r = matching.pos_in_grid(s["grid"], *uv[keys[k]])
        cell = c * s["grid"]["rows"] + r
        assert start[cell] <= k < start[cell + 1]


def test_argument_errors_and_empty_calls(host):
    s = ms.quirk_scenes()["two_to_one"]
    a = list(ms.args(s))

    def bad_grid(**kw):
        with pytest.raises(capi.DeftriError) as e:
            host.match_for_initialization(dict(s["grid"], **kw), *a[1:])
        assert e.value.code == _abi.DEFTRI_E_ARG and len(str(e.value)) > 25
        return str(e.value)

    assert "nGridCols" in bad_grid(cols=0)
    bad_grid(rows=-3)
    assert "max <= min" in bad_grid(max_col=0.0)
    bad_grid(max_row=-1.0)
    assert "nScales" in bad_grid(n_scales=0)
    for which, arr in ((2, [0, 8]), (2, [-1, 0]), (5, [9])):
        b = list(a); b[which] = np.array(arr, np.int32)
        with pytest.raises(capi.DeftriError, match="octave") as e:
            host.match_for_initialization(*b)
        assert e.value.code == _abi.DEFTRI_E_ARG
    # null required pointers, straight through the C entry
    lib, g = host.lib, _abi.FeatureGrid(**s["grid"])
    nm = C.c_int32(7)
    uv = s["uv1"].ctypes.data_as(C.POINTER(C.c_float)); oc = s["octave1"].ctypes.data_as(C.POINTER(C.c_int32))
    de = s["desc1"].ctypes.data_as(C.POINTER(C.c_uint8)); out = np.zeros(2, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.deftri_match_for_initialization(host.h, None, 2, uv, oc, de, 2, uv, oc, de, 100, 25.0, out, None, None,
                                               C.byref(nm)) == _abi.DEFTRI_E_ARG
    assert b"null" in lib.deftri_last_error(host.h)
    assert lib.deftri_match_for_initialization(host.h, C.byref(g), 2, uv, oc, None, 2, uv, oc, de, 100, 25.0, out, None, None,
                                               C.byref(nm)) == _abi.DEFTRI_E_ARG
    assert lib.deftri_match_for_initialization(host.h, C.byref(g), 2, uv, oc, de, 2, uv, oc, de, 100, 25.0, out, None, None,
                                               None) == _abi.DEFTRI_E_ARG
    # best_dist / second_dist may be NULL
    assert lib.deftri_match_for_initialization(host.h, C.byref(g), 2, uv, oc, de, 2, uv, oc, de, 100, 25.0, out, None, None,
                                               C.byref(nm)) == 0 and nm.value == 2
    # zero sizes: 0, every entry -1
    e2 = (s["uv2"][:0], s["octave2"][:0], s["desc2"][:0])
    m, best, second, n = host.match_for_initialization(a[0], a[1], a[2], a[3], *e2, 100, 25.0)
    assert list(m) == [-1, -1] and list(best) == [255, 255] and n == 0
    m, _, _, n = host.match_for_initialization(a[0], s["uv1"][:0], s["octave1"][:0], s["desc1"][:0], a[4], a[5], a[6], 100, 25.0)
    assert m.shape == (0,) and n == 0
    # fewer than 8 matches: cv::kmeans throws in the reference
    uv1, uv2, k1, k2, T1w, T2w, _ = ts.scene(20, nans=0)
    with pytest.raises(capi.DeftriError, match="kmeans") as e:
        host.epipolar_inliers(uv1[:7], uv2[:7], k1, k2, T1w, T2w, EPI_TH)
    assert e.value.code == _abi.DEFTRI_E_ARG
    assert host.epipolar_inliers(uv1[:8], uv2[:8], k1, k2, T1w, T2w, EPI_TH)[0].shape == (8,)
    assert host.lib.deftri_sizeof(14) == C.sizeof(_abi.FeatureGrid) and host.lib.deftri_sizeof(13) == -1


@pytest.mark.parametrize("n", [120, 257])
def test_epipolar_host_loop_against_fp32_restatement(host, n):
    uv1, uv2, k1, k2, T1w, T2w, _ = ts.scene(n, nans=0)
    inl64, err64, _ = matching.epipolar_inliers(uv1, uv2, k1, k2, T1w, T2w, EPI_TH, np.float64)
    # the scene decides nothing within rel 1e-3 of the threshold, and both classes hold 10 % at least
    assert (np.abs(err64 - EPI_TH) > 1e-3 * EPI_TH).all() and 0.1 * n <= inl64.sum() <= 0.9 * n
    inl, err, score = matching.epipolar_inliers(uv1, uv2, k1, k2, T1w, T2w, EPI_TH, np.float32)
    hin, herr, hscore = host.epipolar_inliers(uv1, uv2, k1, k2, T1w, T2w, EPI_TH)
    print(n, score, np.abs(herr - err).max(), np.abs(herr - err64).max())
    assert np.array_equal(hin, inl) and hscore == score == int(inl64.sum())
    assert np.abs(herr.astype(np.float64) - err.astype(np.float64)).max() <= 2e-6
    # a NaN pixel is no inlier
    uv1n = uv1.copy(); uv1n[3] = np.nan
    assert not host.epipolar_inliers(uv1n, uv2, k1, k2, T1w, T2w, 10.0)[0][3]
    # every fifth correspondence is moved across the epipolar line: its error grows by the 6 px or more
    moved = np.arange(n) % 5 == 4
    clean = ts.scene(n, nans=0, offsets=False)
    e_clean = matching.epipolar_inliers(clean[0], clean[1], k1, k2, T1w, T2w, EPI_TH, np.float64)[1]
    assert (np.abs(err64[moved] - e_clean[moved]) > 0.004).all() and np.allclose(err64[~moved & (np.arange(n) % 10 != 0)],
                                                                                 e_clean[~moved & (np.arange(n) % 10 != 0)])


def test_settings_and_keyframe_additions():
    st = Settings(text="FeatureGrid.nGridCols: 64\nFeatureGrid.nGridRows: 48\nFeatureExtractor.nFeatures: 1000\n"
                       "Epipolar.th: 0.002\nMatching.initialization: 50\nMatching.initialization.radius: 25\n"
                       "Triangulation.minMatches: 100\nCamera.cols: 1440\nCamera.rows: 1080\n"
                       "FeatureExtractor.nScales: 8\nFeatureExtractor.fScaleFactor: 1.2\n")
    assert (st.grid_cols, st.grid_rows, st.n_features, st.matching_init_th) == (64, 48, 1000, 50)
    assert (st.epipolar_th, st.matching_init_radius, st.min_matches, st.has_distortion) == (0.002, 25.0, 100.0, False)
    g = matching.feature_grid(st)
    assert g == dict(ms.REALCOLON)
    empty = Settings(text="")
    assert (empty.grid_cols, empty.epipolar_th, empty.min_matches, empty.has_distortion) == (0, 0.0, 0.0, False)
    with pytest.raises(ValueError, match="Camera.k1"):
        matching.feature_grid(Settings(text="Camera.k1: -0.28\nCamera.cols: 752\n"))
    T = ts.poses()[0]
    kf = KeyFrame(0, T, ts.KB8_1, 3, np.ones(8, np.float32))
    assert kf.descriptors is None
    kf = KeyFrame(0, T, ts.KB8_1, 3, np.ones(8, np.float32), descriptors=np.arange(96) % 256)
    assert kf.descriptors.shape == (3, 32) and kf.descriptors.dtype == np.uint8
    with pytest.raises(ValueError, match="Camera.k1"):
        mapping.monocular_map_initialization_from_features(None, kf, kf, Settings(text="Camera.k1: 0.1\n"))
