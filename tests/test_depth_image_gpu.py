"""Real-image input on the device: k_depth_sample against the host function bit for bit, graphs and
arapOptimization whose depth measurements come from the keyframes' depth images, the image
measurements (measureRelativeMapErrors with images, measureRealAbsoluteMapErrors) against the numpy
restatement (tests/depth_image_ref.py), and the sampling cache over a deformationOptimization.

Bands.  Relative errors: rel 1e-9 (fp64 sums), counts exact.  Real absolute errors: counts, n_points
and the divisors exact; average_movement / average_error / rmse rel 1e-6 against the reference's
sequential float32 accumulation.  scale1, scale2 and the up-to-scale figure are float sums of ratios
that then divide every point, so their band is measured, not derived: S = the spread between the
restatement with float32 sequential sums and with fp64 fixed-tree sums on the same inputs, and the band
is 2 S + rel 1e-6 (the device's tree is a third legal order).  S measured on the CPU for these maps
(relative): 1 match 0 / 0 / 0 (scale1 / scale2 / up-to-scale), 65 matches 0 / 0 / 1.2e-7, 257 matches
3.0e-7 / 0 / 3.0e-7, three keyframes x 200 matches 0 / 1.1e-7 / 3.6e-7."""
import copy

import numpy as np
import pytest

from conftest import GOLDEN
from deftri import capi, metrics, optimization, sim
from deftri.problem import Problem
from deftri.settings import Settings
from oracle import graph_ref, oracle
import depth_image_ref as ref

pytestmark = pytest.mark.gpu
SIGMA = np.float32(0.003)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def two_view():
    m, _ = sim.simulate_two_view(n=300, seed=3)
    return ref.synthetic_images(m, (560, 640), seed=7)


@pytest.fixture(scope="module")
def three_view():
    m, _ = sim.simulate_multi_view(n=200, k=3, seed=4)
    return ref.synthetic_images(m, (300, 330), seed=8)


@pytest.fixture(scope="module")
def dev():
    with capi.Context(0) as ctx:
        yield ctx


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_device_sampler_equals_host(dev, n):
    rows, cols = 33, 17
    rng = np.random.default_rng(n)
    img = (10 + 5 * rng.random((rows, cols))).astype(np.float32)
    uv = np.column_stack([rng.uniform(-1, cols + 1, n), rng.uniform(-1, rows + 1, n)]).astype(np.float32)
    if n >= 63:                      # the edges too: spill, last row, out of range, negative, NaN
        uv[:8] = [[cols - 1, 0], [cols - 0.5, 3], [2, rows - 1], [cols, 1], [1, rows], [-1, 2], [np.nan, 2], [cols - 1, rows - 2]]
    with capi.Context(-1) as host:
        for ctx in (host, dev):
            ctx.set_depth_images([(3, img, 1.5, [1, 1, 0, 0])])
        for scaled in (True, False):
            dh, sh = host.depth_measure(3, uv, scaled)
            dd, sd = dev.depth_measure(3, uv, scaled)
            assert np.array_equal(sh, sd)
            assert np.array_equal(_bits(dh[sh == 0]), _bits(dd[sd == 0]))
            assert np.isnan(dd[sd != 0]).all()
    dev.set_depth_images([])


@pytest.mark.parametrize("which", ["two_view", "three_view"])
def test_device_graph_equals_host_graph(dev, which, request):
    m = request.getfixturevalue(which)
    with capi.Context(-1) as host:
        ph = host.build_graph(m, 1.0, 2e5, SIGMA)
    pd = dev.build_graph(m, 1.0, 2e5, SIGMA)
    for f in ("points", "tg", "scales", "cam_kb8", "cam_pose", "rep_point", "rep_cam", "rep_obs", "rep_info", "dep_point",
              "dep_scale", "dep_cam", "dep_meas", "dep_info", "arap_pts", "arap_pair", "arap_rot", "arap_w", "rot",
              "pair_area", "pair_info"):
        assert np.array_equal(getattr(ph, f), getattr(pd, f)), f
    assert np.array_equal(_bits(ph.dep_meas), _bits(pd.dep_meas))
    up, sa = dev.depth_image_stats()
    # the same map again: nothing sent, nothing sampled
    dev.build_graph(m, 1.0, 2e5, SIGMA)
    assert dev.depth_image_stats() == (up, sa)


def test_arap_optimization_with_images_vs_oracle(two_view):
    m, m_ref = copy.deepcopy(two_view), copy.deepcopy(two_view)
    # the oracle's graph from a map whose depth[j] names the row, the restated image lookups substituted
    kw, info = graph_ref.build_arap_graph(ref.tagged(m_ref), 1.0, 2e5, SIGMA)
    kw["dep_meas"] = ref.dep_meas_from_tags(m_ref, kw["dep_meas"])
    sol = oracle.solve_lm(Problem(**kw), 10, analytic=False)
    metrics.apply_solution(m_ref, [info["point_ids"][k] for k in range(len(sol["points"]))], sol["points"])
    upd = optimization.arapOptimization(m, 1.0, 50.0, 2e5, 0.0, 0.0, SIGMA, 10)
    assert upd > 0
    assert abs(metrics.pixels_stand_dev(m)["desv"] - metrics.pixels_stand_dev(m_ref)["desv"]) < 1e-4
    assert m.keyframes[0].estimated_depth_scale == pytest.approx(sol["scales"][0], rel=1e-6, abs=1e-9)
    assert m.keyframes[1].estimated_depth_scale == pytest.approx(sol["scales"][1], rel=1e-6, abs=1e-9)
    # and it is not the per-index problem
    assert not np.array_equal(kw["dep_meas"], graph_ref.build_arap_graph(two_view, 1.0, 2e5, SIGMA)[0]["dep_meas"])


def _check_rel(m):
    got = metrics.measureRelativeMapErrors(m)
    want = ref.relative(m)
    assert len(got) == len(want) > 0
    for g, r in zip(got, want):
        for k in ("kf1", "kf2", "reported", "valid_pairs", "n_matches"):
            assert g[k] == r[k], k
        for k in ("rel_error", "depth_error", "global_t_error", "area"):
            print(k, g[k], r[k])
            assert g[k] == pytest.approx(r[k], rel=1e-9, abs=1e-300), k
    return got


def test_relative_errors_with_images(two_view, three_view):
    from deftri.mapmodel import SE3f, mat_from_quat
    from measurements_ref import relative as relative_per_index
    got = _check_rel(two_view)
    # the images, not the per-index vector
    assert got[-1]["depth_error"] != pytest.approx(relative_per_index(two_view)[-1]["depth_error"], rel=1e-6)
    m = copy.deepcopy(three_view)
    q = np.array([0.01, 0.02, -0.015, 1.0]); q /= np.linalg.norm(q)
    m.insert_global_T(0, 1, SE3f(mat_from_quat(q).astype(np.float32), np.array([0.002, 0.001, -0.003], np.float32)))
    _check_rel(m)
    next(iter(m.keyframes.values())).set_depth_image(None)          # a mixed map
    _check_rel(m)


def _keep_matches(m, count):
    """Leave the first `count` slots of keyframe 0 observed."""
    kf = m.keyframes[0]
    for i, mp in enumerate(kf.map_points):
        if i >= count and mp is not None and m.is_map_point_in_keyframe(mp.id, kf.id) >= 0:
            m.remove_observation(kf.id, mp.id)
    return m


def _check_real_abs(m, n_points):
    got = metrics.measureRealAbsoluteMapErrors(m)
    r32, r64 = ref.real_absolute(m, "f32"), ref.real_absolute(m, "f64")
    print(got, r32, r64)
    assert got["point_count"] == r32["point_count"] == len(m.map_points)
    assert got["n_points"] == r32["n_points"] == n_points
    for k in ("average_movement", "average_error", "rmse"):
        assert got[k] == pytest.approx(r32[k], rel=1e-6), k
    for k in ("scale1", "scale2", "average_up_to_scale_error"):
        S = abs(r32[k] - r64[k])
        assert abs(got[k] - r32[k]) <= 2 * S + 1e-6 * abs(r32[k]), (k, got[k], r32[k], S)


@pytest.mark.parametrize("count", [1, 65, 257])
def test_real_absolute_errors(two_view, count):
    _check_real_abs(_keep_matches(copy.deepcopy(two_view), count), count)


def test_real_absolute_errors_three_keyframes(three_view):
    _check_real_abs(three_view, 600)                 # three pairs x 200: the accumulators carry across pairs
    # a keyframe without an image: the reference throws
    m = copy.deepcopy(three_view)
    m.keyframes[1].set_depth_image(None)
    with pytest.raises(capi.DeftriError, match="keyframe 1"):
        metrics.measureRealAbsoluteMapErrors(m)


def test_deformation_optimization_samples_once_per_keyframe(two_view):
    m = copy.deepcopy(two_view)
    st = Settings(path=GOLDEN / "sim_default" / "settings.yaml")
    st.selection, st.weights_selection, st.depth_weight = "twoOptimizations", "nlopt", 3.0
    st.n_optimizations, st.nlopt_iterations, st.n_iterations = 2, 6, 5
    with capi.Context(0) as ctx:
        r = ctx.deformation_optimization(m, st)
        assert r["rounds"] == 2 and r["arap_calls"] >= 2 + 2
        assert ctx.depth_image_stats() == (2, 2)     # uploads = images, samplings = keyframes
        assert ctx.graph_stats()[0] + ctx.graph_stats()[1] > 0
