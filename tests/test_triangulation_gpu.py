"""Triangulation on the device for every (Triangulation.method, seed.location) the reference defines:
k_triangulate (deftri_triangulate), k_reconstruct_points (deftri_reconstruct_points), k_init_depth_scales
(deftri_init_depth_scales) and deftri.mapping.monocular_map_initialization, against the host
restatements (deftri.sim.triangulate_pair, deftri.mapping).

Bands.  Points: rel 1e-4 against the fp64 restatement, the band test_gpu_parity.py's
test_triangulate_nrslam_device uses for this arithmetic (float ulps of the Newton unprojection and
sin / cos / sqrt, amplified by ~1 / parallax).  cos_parallax: 1e-6 absolute (a float cosine resolves
6e-8).  parallax_deg: rel 1e-3 (acos near 1 amplifies the cosine's ulps).  Statuses, valid flags, keep
flags and counters: equal to the fp32 restatement's, on scenes whose fp64 restatement decides nothing
within rel 1e-3 of a threshold (triangulation_scene.margins_ok).  Depth scales: rel 1e-12 against the
host's sequential fp64 sum (200 positive terms: n * 2^-53 = 2e-14, with room for the order of the
workgroup partials)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from deftri import _abi, capi, mapping, sim
from deftri.mapmodel import KeyFrame, Map, SE3f
from deftri.settings import Settings
import depth_image_ref as ref
import triangulation_scene as ts

gpu = pytest.mark.gpu
F64 = np.float64
OTHER_SEEDS = [("NRSLAM", "TwoPoints"), ("NRSLAM", "InRays"), ("Classic", "TwoPoints"), ("Classic", "InRays")]


def _rel(a, b):
    return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)


@pytest.fixture(scope="module")
def sim_keyframes():
    out = {}
    for n in (120, 257, 1000):
        m, _ = sim.simulate_two_view(n=n, seed=3, scale_scene=n > 257)
        out[n] = (m.keyframes[0], m.keyframes[1])
    return out


def _same_bits(got, want):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


@gpu
@pytest.mark.parametrize("n", [120, 257])
def test_nrslam_far_points_is_bit_identical(gpu_ctx, n):
    """257 = one full 256-thread block and one thread of the next.

    tests/golden/triangulate_nrslam_far.npz holds what deftri_triangulate_nrslam returned on an MI355X at
    commit 8a97c29, the last one where it ran a kernel of its own (k_triangulate_nrslam), for the two
    scenes simulate_two_view(n, seed=3), with the exact fp32 inputs it was given.  The C entry, its
    Python wrapper and (NRSLAM, FarPoints) of deftri_triangulate must all return those bits."""
    g = np.load(GOLDEN / "triangulate_nrslam_far.npz")
    uv1, uv2, k1, k2, Ta, Tb = (g[f"{key}_{n}"] for key in ("uv1", "uv2", "kb8_1", "kb8_2", "T1w", "T2w"))
    want = (g[f"x3d_1_{n}"], g[f"x3d_2_{n}"], g[f"valid_{n}"])
    assert all(a.dtype == np.float32 for a in (uv1, uv2, k1, k2, Ta, Tb)) and uv1.shape == (n, 2)
    assert want[2].sum() > 0.9 * n
    T1w, T2w = SE3f(Ta[:, :3], Ta[:, 3]), SE3f(Tb[:, :3], Tb[:, 3])
    np.testing.assert_array_equal(capi._pose34(T1w), Ta)
    args = (uv1, uv2, k1, k2, T1w, T2w)
    _same_bits(gpu_ctx.triangulate_nrslam(*args), want)
    _same_bits(gpu_ctx.triangulate(*args, method="NRSLAM", location="FarPoints"), want)
    _same_bits(gpu_ctx.triangulate(*args, method="not a method"), want)        # an unknown method is NRSLAM
    # the C entry itself
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    x1 = np.zeros((n, 3), np.float32); x2 = np.zeros((n, 3), np.float32); v = np.zeros(n, np.uint8)
    rc = gpu_ctx.lib.deftri_triangulate_nrslam(gpu_ctx.h, n, fp(uv1), fp(uv2), fp(k1), fp(k2), fp(Ta), fp(Tb), 0.9998, fp(x1),
                                               fp(x2), v.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == 0
    _same_bits((x1, x2, v.astype(bool)), want)


@gpu
@pytest.mark.parametrize("k", [1, 255, 256])
def test_prefix_of_correspondences_is_bit_identical(gpu_ctx, sim_keyframes, k):
    """Every correspondence is one thread's work, independent of n: a call on the first k equals rows [:k]
    of the call on all 257.  k straddles the 256-thread block and the 256-byte padding of the uint8 piece
    of the call's device arena: pieces that overlap or are mis-sized break this."""
    kf0, kf1 = sim_keyframes[257]
    rest = (kf0.kb8, kf1.kb8, kf0.pose, kf1.pose)
    uv1, uv2 = np.asarray(kf0.keypoints, np.float32), np.asarray(kf1.keypoints, np.float32)
    full = gpu_ctx.triangulate(uv1, uv2, *rest)
    _same_bits(gpu_ctx.triangulate(uv1[:k], uv2[:k], *rest), [a[:k] for a in full])
    kw = dict(depth_limit=1e3, checks=True)
    full = gpu_ctx.reconstruct_points(uv1, uv2, *rest, **kw)[:4]
    assert (full[2] == 0).any()                               # the points and cosines compared are real ones
    _same_bits(gpu_ctx.reconstruct_points(uv1[:k], uv2[:k], *rest, **kw)[:4], [a[:k] for a in full])


@gpu
@pytest.mark.parametrize("n", [120, 1000])
@pytest.mark.parametrize("method,location", OTHER_SEEDS)
def test_other_seeds_match_host(gpu_ctx, sim_keyframes, method, location, n):
    kf0, kf1 = sim_keyframes[n]
    x1, x2, v = gpu_ctx.triangulate(kf0.keypoints, kf1.keypoints, kf0.kb8, kf1.kb8, kf0.pose, kf1.pose, method=method,
                                    location=location)
    _, _, refv = sim.triangulate_simulated(kf0.kb8, kf1.kb8, kf0.keypoints, kf1.keypoints, kf0.pose, kf1.pose, method=method,
                                           location=location)
    r64 = mapping.reconstruct_points(kf0.keypoints, kf1.keypoints, kf0.kb8, kf1.kb8, kf0.pose, kf1.pose, method, location,
                                     np.inf, False, 0.0, F64)
    assert v.sum() > 0.9 * n
    np.testing.assert_array_equal(v, refv)
    for a, b in ((x1, r64["x3d_1"]), (x2, r64["x3d_2"])):
        d = _rel(a[v].astype(F64), b[v])
        print(method, location, n, d.max())
        assert d.max() < 1e-4, d.max()
    if location == "TwoPoints":
        np.testing.assert_array_equal(x1, x2)
    # Classic has no FarPoints branch: its else is the in-rays seed
    if (method, location) == ("Classic", "InRays"):
        far = gpu_ctx.triangulate(kf0.keypoints, kf1.keypoints, kf0.kb8, kf1.kb8, kf0.pose, kf1.pose, method="Classic",
                                  location="FarPoints")
        np.testing.assert_array_equal(far[0], x1)
        np.testing.assert_array_equal(far[1], x2)


@gpu
def test_undefined_methods_are_errors(gpu_ctx, sim_keyframes):
    kf0, kf1 = sim_keyframes[120]
    args = (kf0.keypoints, kf1.keypoints, kf0.kb8, kf1.kb8, kf0.pose, kf1.pose)
    with pytest.raises(capi.DeftriError, match=r"Geometry\.cc:155-186") as e:
        gpu_ctx.triangulate(*args, method="ORBSLAM")
    assert e.value.code == _abi.DEFTRI_E_ARG
    with pytest.raises(capi.DeftriError, match=r"CameraModel\.h:128-135") as e:
        gpu_ctx.triangulate(*args, method="DepthMeasurement", location="TwoPoints")
    assert e.value.code == _abi.DEFTRI_E_ARG
    with pytest.raises(capi.DeftriError, match=r"Geometry\.cc:155-186") as e:
        gpu_ctx.reconstruct_points(*args, method="ORBSLAM", depth_limit=1.0)
    assert e.value.code == _abi.DEFTRI_E_ARG


def test_bad_enums_and_null_pointers_are_errors():
    """The C entry points themselves (a host-only context: the argument checks come first)."""
    lib = capi.load()
    with capi.Context(-1) as ctx:
        f = np.zeros(12, np.float32)
        p = f.ctypes.data_as(C.POINTER(C.c_float))
        v = np.zeros(1, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
        for method, loc in ((7, 0), (-1, 2), (1, 3), (1, -1)):
            assert lib.deftri_triangulate(ctx.h, 1, method, loc, p, p, p, p, p, p, 0.9998, p, p, v) == _abi.DEFTRI_E_ARG
        assert lib.deftri_triangulate(ctx.h, 1, 1, 2, None, p, p, p, p, p, 0.9998, p, p, v) == _abi.DEFTRI_E_ARG
        assert lib.deftri_triangulate(ctx.h, -1, 1, 2, p, p, p, p, p, p, 0.9998, p, p, v) == _abi.DEFTRI_E_ARG
        rep = _abi.ReconstructReport()
        prm = _abi.ReconstructParams(method=1, location=5)
        assert lib.deftri_reconstruct_points(ctx.h, 1, p, p, p, p, p, p, C.byref(prm), p, p, v, p, C.byref(rep)) == _abi.DEFTRI_E_ARG
        assert lib.deftri_reconstruct_points(ctx.h, 1, p, p, p, p, p, p, None, p, p, v, p, C.byref(rep)) == _abi.DEFTRI_E_ARG
        s = C.c_double(); npts = C.c_int64()
        assert lib.deftri_init_depth_scales(ctx.h, 0, 1, 1, p, p, p, p, p, p, p, p, 0.9998, v, None, C.byref(s),
                                            C.byref(npts)) == _abi.DEFTRI_E_ARG


def test_host_only_context_has_no_device():
    uv1, uv2, k1, k2, T1w, T2w, _ = ts.scene(5, seed=0, nans=0)
    with capi.Context(-1) as ctx:
        for call in (lambda: ctx.triangulate(uv1, uv2, k1, k2, T1w, T2w, method="Classic", location="InRays"),
                     lambda: ctx.reconstruct_points(uv1, uv2, k1, k2, T1w, T2w, depth_limit=1.0),
                     lambda: ctx.init_depth_scales(0, 1, uv1, uv2, np.zeros((5, 3)), np.zeros((5, 3)), k1, k2, T1w, T2w)):
            with pytest.raises(capi.DeftriError) as e:
                call()
            assert e.value.code == _abi.DEFTRI_E_NODEVICE


@gpu
def test_empty_and_single_correspondence(gpu_ctx):
    uv1, uv2, k1, k2, T1w, T2w, _ = ts.scene(5, seed=0, nans=0)
    x1, x2, v = gpu_ctx.triangulate(uv1[:0], uv2[:0], k1, k2, T1w, T2w, method="Classic", location="InRays")
    assert x1.shape == (0, 3) and x2.shape == (0, 3) and v.shape == (0,)
    x1, x2, st, cosp, rep = gpu_ctx.reconstruct_points(uv1[:0], uv2[:0], k1, k2, T1w, T2w, depth_limit=1.0)
    assert x1.shape == (0, 3) and st.shape == (0,) and cosp.shape == (0,)
    assert all(val == 0 for val in rep.values())
    for method, location in OTHER_SEEDS + [("NRSLAM", "FarPoints")]:
        x1, x2, v = gpu_ctx.triangulate(uv1[:1], uv2[:1], k1, k2, T1w, T2w, method=method, location=location)
        r64 = mapping.reconstruct_points(uv1[:1], uv2[:1], k1, k2, T1w, T2w, method, location, np.inf, False, 0.0, F64)
        assert v.tolist() == [True]
        assert _rel(x1.astype(F64), r64["x3d_1"]).max() < 1e-4 and _rel(x2.astype(F64), r64["x3d_2"]).max() < 1e-4
    x1, x2, st, cosp, rep = gpu_ctx.reconstruct_points(uv1[:1], uv2[:1], k1, k2, T1w, T2w, depth_limit=1.0)
    assert st.tolist() == [0] and rep["n_triangulated"] == 2 and rep["accepted"] == 0 and rep["parallax_deg"] > 0


# ---- reconstructPoints -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def all_status_scene():
    return ts.scene(300, seed=0)


RECONSTRUCT = [("NRSLAM", "FarPoints", True), ("Classic", "InRays", True), ("DepthMeasurement", "TwoPoints", False)]


def _check_reconstruct(ctx, scene, sel, method, location, limit, checks, min_parallax=0.9998):
    uv1, uv2, k1, k2, T1w, T2w, _ = scene
    uv1, uv2 = uv1[sel], uv2[sel]
    kw = dict(method=method, location=location, depth_limit=limit, checks=checks, min_parallax=min_parallax)
    r64 = mapping.reconstruct_points(uv1, uv2, k1, k2, T1w, T2w, dtype=F64, **kw)
    r32 = mapping.reconstruct_points(uv1, uv2, k1, k2, T1w, T2w, **kw)
    assert ts.margins_ok(r64, limit, checks)                  # status equality is a fair demand
    x1, x2, st, cosp, rep = ctx.reconstruct_points(uv1, uv2, k1, k2, T1w, T2w, **kw)
    print(method, location, len(uv1), np.bincount(st, minlength=6), rep)
    np.testing.assert_array_equal(st, r32["status"])
    np.testing.assert_array_equal(st, r64["status"])
    kept = st == 0
    for a, b in ((x1, r64["x3d_1"]), (x2, r64["x3d_2"])):
        d = _rel(a[kept].astype(F64), b[kept])
        print("  points", d.max())
        assert d.max() < 1e-4, d.max()
    fin = st != 1
    dc = np.abs(cosp[fin].astype(F64) - r64["cos_parallax"][fin])
    print("  cos", dc.max())
    assert dc.max() < 1e-6
    want = r32["report"]
    for k in ("n_triangulated", "n_nonfinite", "n_depth1", "n_err1", "n_depth2", "n_err2", "accepted"):
        assert rep[k] == want[k], k
    assert rep["parallax_deg"] == pytest.approx(r64["report"]["parallax_deg"], rel=1e-3)
    return st, rep, r64


@gpu
@pytest.mark.parametrize("method,location,checks", RECONSTRUCT)
def test_reconstruct_points_matches_host(gpu_ctx, all_status_scene, method, location, checks):
    uv1, uv2, k1, k2, T1w, T2w, _ = all_status_scene
    free = mapping.reconstruct_points(uv1, uv2, k1, k2, T1w, T2w, method, location, np.inf, False, 0.0, F64)
    limit = ts.depth_limit_for(method, free)
    # n = 300: more than 50 kept, the 50th smallest cosine decides
    st, rep, r64 = _check_reconstruct(gpu_ctx, all_status_scene, np.arange(300), method, location, limit, checks)
    kept, lost = np.flatnonzero(st == 0), np.flatnonzero(st != 0)
    assert len(kept) > 51 and rep["accepted"] == 1
    assert rep["parallax_deg"] == pytest.approx(np.degrees(np.arccos(np.sort(r64["cos_parallax"][kept])[50])), rel=1e-3)
    if method == "NRSLAM":
        assert (np.bincount(st, minlength=6) >= 3).all()
    # 30 correspondences, 22 of them kept: index kept - 1, the largest kept cosine
    sel = np.sort(np.concatenate([kept[:22], lost[:8]]))
    st, rep, r64 = _check_reconstruct(gpu_ctx, all_status_scene, sel, method, location, limit, checks)
    assert (st == 0).sum() == 22 and rep["n_triangulated"] == 44 and rep["accepted"] == 1
    assert rep["parallax_deg"] == pytest.approx(np.degrees(np.arccos(r64["cos_parallax"][st == 0].max())), rel=1e-3)
    # fewer than 13 kept: under 25 points, not accepted
    sel = np.sort(np.concatenate([kept[:8], lost[:8]]))
    st, rep, _ = _check_reconstruct(gpu_ctx, all_status_scene, sel, method, location, limit, checks)
    assert rep["n_triangulated"] == 16 and rep["accepted"] == 0 and rep["parallax_deg"] > 0
    # enough points, not enough parallax
    _, rep, _ = _check_reconstruct(gpu_ctx, all_status_scene, np.arange(300), method, location, limit, checks, min_parallax=60.0)
    assert rep["accepted"] == 0


# ---- the initial depth scales and the map of two real keyframes ------------------------------------

N_REAL = 200
SHAPE = (64, 64)


def _real_pair():
    """Two keyframes over 64 x 64 depth images: keyframe 1's keypoints permuted (matches is the
    permutation), four keypoints over zero depth and three at x <= 0.1."""
    uv1, uv2, k1, k2, T1w, T2w, info = ts.scene(N_REAL, seed=1, kb8_1=ts.KB8_SMALL_1, kb8_2=ts.KB8_SMALL_2, offsets=False,
                                                nans=0)
    uv1 = uv1.copy()
    uv1[[20, 90, 160], 0] = [0.05, 0.0999, 0.0]              # outside (0.1, 1500), inside the image
    matches = np.random.default_rng(3).permutation(N_REAL)
    kp2 = np.zeros_like(uv2); z2 = np.zeros(N_REAL)
    kp2[matches] = uv2; z2[matches] = info["z2"]
    inv_s2 = sim.inv_sigma2_table(8, 1.2)
    kf_ref = KeyFrame(0, T1w, k1, N_REAL, inv_s2, uv1, np.zeros(N_REAL, np.int32), info["z1"])
    kf_cur = KeyFrame(1, T2w, k2, N_REAL, inv_s2, kp2, np.zeros(N_REAL, np.int32), z2)
    m = Map()
    m.insert_keyframe(kf_ref); m.insert_keyframe(kf_cur)
    ref.synthetic_images(m, SHAPE, seed=5)
    for kf, uv in ((kf_ref, uv1[[11, 47]]), (kf_cur, uv2[[73, 130]])):
        img = kf.depth_image.copy()
        for x, y in uv:
            img[int(y):int(y) + 2, int(x):int(x) + 2] = 0.0
        kf.set_depth_image(img, kf.image_depth_scale, kf.ph)
    return kf_ref, kf_cur, matches, uv1, uv2, info


@pytest.fixture(scope="module")
def real_pair(gpu_ctx):
    yield _real_pair()
    gpu_ctx.set_depth_images([])


def _ref_sampler(kf, uv, scaled):
    return ref.sample(kf.depth_image, uv, kf.image_depth_scale, scaled)


@gpu
@pytest.mark.parametrize("min_cos", [0.9998, 17.5])
def test_init_depth_scales_matches_host(gpu_ctx, real_pair, min_cos):
    """min_cos 17.5: the reference compares the parallax in degrees with it, so it splits this scene."""
    kf_ref, kf_cur, matches, uv1, uv2, info = real_pair
    world = info["world"].astype(np.float32)
    x1, x2 = world + np.float32(1e-4), world - np.float32(1e-4)
    gpu_ctx.set_depth_images([(kf.id, kf.depth_image, kf.image_depth_scale, kf.ph) for kf in (kf_ref, kf_cur)])
    keep, s1, s2, npts = gpu_ctx.init_depth_scales(0, 1, uv1, uv2, x1, x2, kf_ref.kb8, kf_cur.kb8, kf_ref.pose, kf_cur.pose,
                                                   min_cos)
    hkeep, h1, h2, hn = mapping.init_depth_scales(kf_ref, kf_cur, uv1, uv2, x1, x2, min_cos, sampler=_ref_sampler)
    print(min_cos, keep.sum(), npts, s1, h1, s2, h2)
    np.testing.assert_array_equal(keep, hkeep)
    assert 7 <= (~keep).sum() < 40 and not keep[[20, 90, 160, 11, 47, 73, 130]].any()   # and neighbours over a zeroed pixel
    assert npts == hn and (npts == keep.sum() if min_cos < 1 else 0 < npts < keep.sum())
    assert s1 == pytest.approx(h1, rel=1e-12) and s2 == pytest.approx(h2, rel=1e-12)
    # the library's own host sampler gives the restatement the same values
    assert mapping.init_depth_scales(kf_ref, kf_cur, uv1, uv2, x1, x2, min_cos)[1:] == (h1, h2, hn)
    # no correspondence passes the degrees test: 0 / 0, NaN as the reference
    keep, s1, s2, npts = gpu_ctx.init_depth_scales(0, 1, uv1, uv2, x1, x2, kf_ref.kb8, kf_cur.kb8, kf_ref.pose, kf_cur.pose, 90.0)
    assert npts == 0 and np.isnan(s1) and np.isnan(s2) and np.array_equal(keep, hkeep)
    keep, s1, s2, npts = gpu_ctx.init_depth_scales(0, 1, uv1[:0], uv2[:0], x1[:0], x2[:0], kf_ref.kb8, kf_cur.kb8, kf_ref.pose,
                                                   kf_cur.pose, min_cos)
    assert keep.shape == (0,) and npts == 0 and np.isnan(s1)


@gpu
def test_init_depth_scales_bad_pixel_leaves_outputs(gpu_ctx, real_pair):
    kf_ref, kf_cur, matches, uv1, uv2, info = real_pair
    world = info["world"].astype(np.float32)
    gpu_ctx.set_depth_images([(kf.id, kf.depth_image, kf.image_depth_scale, kf.ph) for kf in (kf_ref, kf_cur)])
    bad = uv2.copy()
    bad[33] = [70.0, 12.5]                                   # x >= cols: the reference throws std::out_of_range
    out = (np.full(N_REAL, 9, np.uint8), np.full(2, -7.0), np.full(1, -5, np.int64))
    with pytest.raises(capi.DeftriError, match=r"keyframe 1 .*\(70, 12\.5\)") as e:
        gpu_ctx.init_depth_scales(0, 1, uv1, bad, world, world, kf_ref.kb8, kf_cur.kb8, kf_ref.pose, kf_cur.pose, out=out)
    assert e.value.code == _abi.DEFTRI_E_ARG
    assert (out[0] == 9).all() and (out[1] == -7.0).all() and out[2][0] == -5
    with pytest.raises(capi.DeftriError, match="keyframe 5") as e:       # no image for that keyframe
        gpu_ctx.init_depth_scales(0, 5, uv1, uv2, world, world, kf_ref.kb8, kf_cur.kb8, kf_ref.pose, kf_cur.pose)
    assert e.value.code == _abi.DEFTRI_E_ARG


@gpu
def test_monocular_map_initialization(gpu_ctx, real_pair):
    kf_ref, kf_cur, matches, uv1, uv2, info = real_pair
    st = Settings(path=GOLDEN / "sim_default" / "settings.yaml")
    st.depth_limit, st.trian_checks = 10.0, False
    for kf in (kf_ref, kf_cur):
        kf.map_points = [None] * N_REAL
    m, rep = mapping.monocular_map_initialization(gpu_ctx, kf_ref, kf_cur, matches, st)
    assert rep["accepted"] == 1 and m is not None and list(m.keyframes) == [0, 1]
    # the same two steps by hand: the device's points, the host's filter and sums
    x1, x2, status, _, _ = gpu_ctx.reconstruct_points(uv1, uv2, kf_ref.kb8, kf_cur.kb8, kf_ref.pose, kf_cur.pose, method="NRSLAM",
                                                      location="FarPoints", depth_limit=10.0, checks=False, min_parallax=st.min_cos)
    tri = np.flatnonzero(status == 0)
    assert len(tri) >= N_REAL - 3
    hkeep, h1, h2, hn = mapping.init_depth_scales(kf_ref, kf_cur, uv1[tri], uv2[tri], x1[tri], x2[tri], st.min_cos,
                                                  sampler=_ref_sampler)
    kept = tri[hkeep]
    assert 0 < len(kept) < len(tri)
    assert len(m.map_points) == 2 * len(kept) == rep["n_map_points"] and rep["n_scale_points"] == hn
    for i in range(N_REAL):
        mp1, mp2 = kf_ref.map_points[i], kf_cur.map_points[i]
        if i not in kept:
            assert mp1 is None and mp2 is None
            continue
        # both slots at index i (Mapping.cc:208-209); the observations at i and matches[i]
        assert np.array_equal(mp1.position, x1[i]) and np.array_equal(mp2.position, x2[i])
        assert m.is_map_point_in_keyframe(mp1.id, 0) == i and m.is_map_point_in_keyframe(mp2.id, 1) == matches[i]
    assert (matches[kept] != kept).any()
    assert kf_ref.estimated_depth_scale == pytest.approx(h1, rel=1e-12)
    assert kf_cur.estimated_depth_scale == pytest.approx(h2, rel=1e-12)
    # the hand-over to the real-keyframe arapOptimization: one iteration runs
    upd, report = gpu_ctx.arap_optimization(m, 1.0, 50.0, 2e5, 0.0, 0.0, np.float32(0.003), 1)
    assert report["iterations"] >= 1 and np.isfinite(upd)
    # a pair without parallax enough is not a map
    st.min_cos = 60.0
    assert mapping.monocular_map_initialization(gpu_ctx, kf_ref, kf_cur, matches, st)[0] is None


@gpu
def test_simulate_two_view_follows_the_seed_location(gpu_ctx):
    """Changing Triangulation.seed.location changes the simulator's map, on the host and on the device."""
    a, _ = sim.simulate_two_view(n=120, seed=3)
    b, _ = sim.simulate_two_view(n=120, seed=3, trian_method="NRSLAM", trian_location="FarPoints")
    c, _ = sim.simulate_two_view(n=120, seed=3, trian_location="InRays")
    assert all(np.array_equal(a.map_points[k].position, b.map_points[k].position) for k in a.map_points)
    assert len(c.map_points) > 200
    assert any(not np.array_equal(a.map_points[k].position, c.map_points[k].position) for k in a.map_points if k in c.map_points)
    kf0, kf1 = c.keyframes[0], c.keyframes[1]
    x1, _, v = gpu_ctx.triangulate(kf0.keypoints, kf1.keypoints, kf0.kb8, kf1.kb8, kf0.pose, kf1.pose, location="InRays")
    pos = np.array([mp.position for mp in kf0.map_points if mp is not None])
    assert v.sum() == len(pos) and _rel(x1[v], pos).max() < 1e-4


# ---- ABI ---------------------------------------------------------------------------------------

def test_new_struct_sizes_match_c(tmp_path):
    """The ctypes mirrors against a C translation unit compiled from include/deftri.h (gcc, as
    tests/test_c_consumer.py compiles its consumer)."""
    lib = capi.load()
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "deftri.h"\nint main(void) {\n'
                   '    printf("%zu %zu %d %d\\n", sizeof(deftri_reconstruct_params), sizeof(deftri_reconstruct_report),\n'
                   '           DEFTRI_TRI_CLASSIC + 10 * DEFTRI_TRI_NRSLAM + 100 * DEFTRI_TRI_ORBSLAM + 1000 * DEFTRI_TRI_DEPTH,\n'
                   '           DEFTRI_LOC_INRAYS + 10 * DEFTRI_LOC_TWOPOINTS + 100 * DEFTRI_LOC_FARPOINTS);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out[:2]] == [C.sizeof(_abi.ReconstructParams), C.sizeof(_abi.ReconstructReport)] == [20, 56]
    assert int(out[2]) == (_abi.DEFTRI_TRI_CLASSIC + 10 * _abi.DEFTRI_TRI_NRSLAM + 100 * _abi.DEFTRI_TRI_ORBSLAM +
                           1000 * _abi.DEFTRI_TRI_DEPTH)
    assert int(out[3]) == _abi.DEFTRI_LOC_INRAYS + 10 * _abi.DEFTRI_LOC_TWOPOINTS + 100 * _abi.DEFTRI_LOC_FARPOINTS
    for name in ("deftri_triangulate", "deftri_reconstruct_points", "deftri_init_depth_scales"):
        assert name in capi.EXPORTED and hasattr(lib, name)
