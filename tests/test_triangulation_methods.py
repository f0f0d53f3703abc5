"""The seeds of useTriangulationMethod (Geometry.cc:216-230) and reconstructPoints
(MonocularMapInitializer.cc:281-395) as host restatements (deftri.sim.triangulate_pair,
deftri.mapping.reconstruct_points): geometric identities in fp64, the Classic closed form against
numpy's SVD, the status histogram of the scene the GPU tests reuse, and the settings keys."""
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN
from deftri import mapping, sim
from deftri.mapmodel import SE3f
from deftri.settings import Settings
import triangulation_scene as ts

F64 = np.float64
DEFINED = [("NRSLAM", "TwoPoints"), ("NRSLAM", "FarPoints"), ("NRSLAM", "InRays"), ("Classic", "TwoPoints"),
           ("Classic", "InRays")]


def sim_like_rays(n=1000, seed=0):
    """Unit rays of a cloud laid out like the simulator's (create_data.py's stds and offset, the
    Simulation.yaml camera centres, camera 2 looking at the first moved point), with 2e-3 of ray noise."""
    rs = np.random.RandomState(seed)
    orig, moved = sim.generate_points(n, seed=seed)
    c1, c2 = np.array([-0.10, 0.02, 0.12]), np.array([0.14, 0.01, 0.06])
    # fp64 poses with rotations orthonormal to fp64 (an SE3f keeps float32 entries)
    u, _, vt = np.linalg.svd(sim.look_at(c2, moved[0]).astype(F64))
    T1w = SimpleNamespace(R=np.eye(3), t=c1)
    T2w = SimpleNamespace(R=u @ vt, t=c2)
    x1 = orig @ T1w.R.astype(F64).T + T1w.t.astype(F64)
    x2 = moved @ T2w.R.astype(F64).T + T2w.t.astype(F64)
    x1 += rs.normal(0, 2e-3, x1.shape) * x1[:, 2:3]
    x2 += rs.normal(0, 2e-3, x2.shape) * x2[:, 2:3]
    return x1 / np.linalg.norm(x1, axis=1, keepdims=True), x2 / np.linalg.norm(x2, axis=1, keepdims=True), T1w, T2w


@pytest.fixture(scope="module")
def rays():
    return sim_like_rays()


def _cam(T, x):
    return x @ T.R.astype(F64).T + T.t.astype(F64)


def _sine(a, b):
    return np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


@pytest.mark.parametrize("method", ["NRSLAM", "Classic", "DepthMeasurement"])
def test_in_rays_points_lie_on_their_rays(rays, method):
    xn1, xn2, T1w, T2w = rays
    for location in ("InRays", "anything else"):          # any other string is the in-rays seed
        x1, x2 = sim.triangulate_pair(xn1, xn2, T1w, T2w, method, location, dtype=F64)
        assert _sine(_cam(T1w, x1), xn1).max() < 1e-9
        assert _sine(_cam(T2w, x2), xn2).max() < 1e-9


@pytest.mark.parametrize("method", ["NRSLAM", "Classic", "DepthMeasurement"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_points_are_one_point(rays, method, dtype):
    xn1, xn2, T1w, T2w = rays
    x1, x2 = sim.triangulate_pair(xn1, xn2, T1w, T2w, method, "TwoPoints", dtype=dtype)
    assert x1.dtype == np.dtype(dtype) and np.isfinite(x1).all()
    np.testing.assert_array_equal(x1, x2)


@pytest.mark.parametrize("method", ["NRSLAM", "DepthMeasurement"])
def test_far_points_mirror_the_two_points_seed(rays, method):
    xn1, xn2, T1w, T2w = rays
    seeds = {loc: sim.triangulate_pair(xn1, xn2, T1w, T2w, method, loc, dtype=F64) for loc in ("InRays", "TwoPoints", "FarPoints")}
    for k in (0, 1):
        want = 2 * seeds["InRays"][k] - seeds["TwoPoints"][k]
        d = np.linalg.norm(seeds["FarPoints"][k] - want, axis=1) / np.linalg.norm(want, axis=1)
        assert d.max() < 1e-12, d.max()
    # the seeds differ: a map built from another location is another map
    assert np.abs(seeds["FarPoints"][0] - seeds["InRays"][0]).max() > 1e-6


def test_classic_far_points_is_the_in_rays_seed(rays):
    xn1, xn2, T1w, T2w = rays
    a = sim.triangulate_pair(xn1, xn2, T1w, T2w, "Classic", "FarPoints", dtype=F64)
    b = sim.triangulate_pair(xn1, xn2, T1w, T2w, "Classic", "InRays", dtype=F64)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_unknown_method_is_nrslam_and_undefined_methods_raise(rays):
    xn1, xn2, T1w, T2w = rays
    a = sim.triangulate_pair(xn1, xn2, T1w, T2w, "SomethingElse", "FarPoints")
    b = sim.triangulate_pair(xn1, xn2, T1w, T2w, "NRSLAM", "FarPoints")
    np.testing.assert_array_equal(a[0], b[0])
    with pytest.raises(ValueError, match=r"Geometry\.cc:155-186"):
        sim.triangulate_pair(xn1, xn2, T1w, T2w, "ORBSLAM", "FarPoints")
    uv = np.zeros((2, 2), np.float32) + 300
    with pytest.raises(ValueError, match=r"Geometry\.cc:155-186"):
        sim.triangulate_simulated(sim.SIM_KB8, sim.SIM_KB8, uv, uv, T1w, T2w, method="ORBSLAM")
    with pytest.raises(ValueError, match=r"CameraModel\.h:128-135"):
        sim.triangulate_simulated(sim.SIM_KB8, sim.SIM_KB8, uv, uv, T1w, T2w, method="DepthMeasurement")


def test_classic_closed_form_matches_svd(rays):
    """n = t x v0 (v0 from the 2x2 A A^T) against col(1) of numpy's fp64 SVD, through the whole seed:
    rel 1e-8 (6e-11 observed).  The scene is ill-conditioned for an fp32 SVD — sigma_1 / sigma_0 is small —
    which is why the device does not run one."""
    xn1, xn2, T1w, T2w = rays
    R21 = T2w.R @ T1w.R.T
    t21 = T2w.t - R21 @ T1w.t
    t = t21 / np.linalg.norm(t21)
    A = np.stack([xn1 @ R21.T, xn2], 1) @ (np.eye(3) - np.outer(t, t))
    sv = np.linalg.svd(A, compute_uv=False)
    assert (sv[:, 1] / sv[:, 0]).max() < 0.1
    for location in ("TwoPoints", "InRays"):
        closed = sim.triangulate_pair(xn1, xn2, T1w, T2w, "Classic", location, dtype=F64)
        svd = sim.triangulate_pair(xn1, xn2, T1w, T2w, "Classic", location, dtype=F64, classic_svd=True)
        for a, b in zip(closed, svd):
            d = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
            print(location, d.max())
            assert d.max() < 1e-8, d.max()


def test_simulated_triangulation_follows_the_settings():
    """Another seed.location gives another map; the default arguments still give today's."""
    rs = np.random.RandomState(2)
    xn1, xn2, T1w, T2w = sim_like_rays(120, seed=2)
    T1w, T2w = SE3f(T1w.R, T1w.t), SE3f(T2w.R, T2w.t)
    uv1 = sim.kb8_project(sim.SIM_KB8, xn1.astype(np.float32)) + rs.normal(0, 0.3, (120, 2)).astype(np.float32)
    uv2 = sim.kb8_project(sim.SIM_KB8, xn2.astype(np.float32)) + rs.normal(0, 0.3, (120, 2)).astype(np.float32)
    base = sim.triangulate_simulated(sim.SIM_KB8, sim.SIM_KB8, uv1, uv2, T1w, T2w)
    same = sim.triangulate_simulated(sim.SIM_KB8, sim.SIM_KB8, uv1, uv2, T1w, T2w, method="NRSLAM", location="FarPoints")
    for a, b in zip(base, same):
        np.testing.assert_array_equal(a, b)
    for method, location in DEFINED:
        if (method, location) == ("NRSLAM", "FarPoints"):
            continue
        x1, x2, valid = sim.triangulate_simulated(sim.SIM_KB8, sim.SIM_KB8, uv1, uv2, T1w, T2w, method=method, location=location)
        assert valid.sum() > 0.9 * 120
        assert np.abs(x1[valid] - base[0][valid]).max() > 1e-6, (method, location)


# ---- reconstructPoints -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def all_status_scene():
    return ts.scene(300, seed=0)


def test_reconstruct_points_scene_has_every_status(all_status_scene):
    uv1, uv2, k1, k2, T1w, T2w, info = all_status_scene
    kw = dict(method="NRSLAM", location="FarPoints", depth_limit=ts.DEPTH_LIMIT, checks=True, min_parallax=0.9998)
    r64 = mapping.reconstruct_points(uv1, uv2, k1, k2, T1w, T2w, dtype=F64, **kw)
    r32 = mapping.reconstruct_points(uv1, uv2, k1, k2, T1w, T2w, **kw)
    hist = np.bincount(r64["status"], minlength=6)
    print(hist)
    assert len(hist) == 6 and (hist >= 3).all(), hist
    assert ts.margins_ok(r64, ts.DEPTH_LIMIT, True)
    np.testing.assert_array_equal(r32["status"], r64["status"])
    # the statuses are the scene's design: the NaN pixels, the layers, then the moved pixels
    assert (r64["status"][np.isnan(uv1[:, 0])] == 1).all()
    ok = ~np.isnan(uv1[:, 0])
    assert (r64["status"][ok & (info["layer"] == 2)] == 2).all()
    assert np.isin(r64["status"][ok & (info["layer"] == 1)], (3, 4)).all()
    assert np.isin(r64["status"][ok & (info["layer"] == 0)], (0, 3, 5)).all()
    kept = r64["status"] == 0
    d = np.linalg.norm(r64["x3d_1"][kept] - info["world"][kept], axis=1)
    assert d.max() < 2e-3                                    # 0.1 px of noise at 0.2 m
    rep = r64["report"]
    assert rep["n_triangulated"] == 2 * hist[0] and rep["accepted"] == 1
    assert [rep[k] for k in ("n_nonfinite", "n_depth1", "n_err1", "n_depth2", "n_err2")] == list(hist[1:])
    cos50 = np.sort(r64["cos_parallax"][kept])[50]
    assert rep["parallax_deg"] == pytest.approx(np.degrees(np.arccos(cos50)), rel=1e-3)


def test_reconstruct_points_checks_off_and_other_seeds(all_status_scene):
    uv1, uv2, k1, k2, T1w, T2w, info = all_status_scene
    r = mapping.reconstruct_points(uv1, uv2, k1, k2, T1w, T2w, "NRSLAM", "FarPoints", ts.DEPTH_LIMIT, False, 0.9998, F64)
    assert set(np.unique(r["status"])) == {0, 1, 2, 4}
    # on-ray seeds reproject onto their pixels, so the reprojection tests never fire.  The poses' float32
    # rotations are orthonormal to ~1e-7 only: up to ~1e-7 rad * 700 px = 1e-4 px, 1e-8 px^2
    r = mapping.reconstruct_points(uv1, uv2, k1, k2, T1w, T2w, "Classic", "InRays", ts.DEPTH_LIMIT, True, 0.9998, F64)
    assert set(np.unique(r["status"])) == {0, 1, 2, 4}
    assert np.nanmax(r["err1"]) < 1e-8 and np.nanmax(r["err2"]) < 1e-8


def test_acceptance_order_statistic():
    cos = np.cos(np.radians(np.linspace(5, 40, 80))).astype(np.float32)      # descending cosines
    st = np.zeros(80, np.uint8)
    rep = mapping.acceptance(st, cos, 0.9998)
    assert rep["n_triangulated"] == 160 and rep["accepted"] == 1
    assert rep["parallax_deg"] == pytest.approx(np.degrees(np.arccos(np.sort(cos)[50])), rel=1e-5)
    rep = mapping.acceptance(st[:30], cos[:30], 0.9998)                      # index kept - 1: the largest cosine
    assert rep["parallax_deg"] == pytest.approx(5.0, rel=1e-4) and rep["accepted"] == 1
    rep = mapping.acceptance(st[:12], cos[:12], 0.9998)                      # 24 < 25 points
    assert rep["accepted"] == 0 and rep["parallax_deg"] > 0
    assert mapping.acceptance(st, cos, 60.0)["accepted"] == 0                # not enough parallax
    assert mapping.acceptance(st, -cos, 0.9998) == dict(rep, n_triangulated=160, parallax_deg=0.0, accepted=0)
    none = mapping.acceptance(np.full(5, 2, np.uint8), cos[:5], 0.9998)
    assert none["n_triangulated"] == 0 and none["accepted"] == 0 and none["parallax_deg"] == 0.0 and none["n_depth1"] == 5


# ---- settings ----------------------------------------------------------------------------------

def test_triangulation_settings_round_trip():
    text = (GOLDEN / "sim_default" / "settings.yaml").read_text()
    st = Settings(text=text)
    assert (st.trian_method, st.trian_location) == ("NRSLAM", "FarPoints")
    assert st.depth_limit == 0.0 and st.trian_checks is False           # absent keys: 0 and not "true"
    st = Settings(text=text.replace('"FarPoints"', '"InRays"').replace('"NRSLAM" #', '"Classic" #') +
                  '\nTriangulation.depthLimit: 0.35\nTriangulation.checks: "true"\n')
    assert (st.trian_method, st.trian_location, st.depth_limit, st.trian_checks) == ("Classic", "InRays", 0.35, True)
    assert Settings(text='Triangulation.checks: "True"').trian_checks is False      # only the string "true"
    for name in ("db_planar_gr_1", "db_gradual_gr_2"):
        assert Settings(path=GOLDEN / name / "settings.yaml").trian_location == "InRays"
