"""TEST INFRASTRUCTURE ONLY: the two-view scene of the triangulation tests (numpy alone).

Points lie in three depth layers in front of camera 1 (z = 0.20, 0.25, 0.32 m, each +-4 mm) and, sideways,
in a central disc or an outer ring; camera 2 stands 7 cm to the side and 4 cm further back, with a
longer focal length.  So with depth_limit = 0.27 the first layer passes both depth tests, the second
fails in view 2 only and the third in view 1, each by centimetres.  Every pixel carries 0.1 px of noise;
every fifth correspondence is also moved across the epipolar line in view 2, by 6 px (the reprojection
test fails in view 2 only: camera 2's focal length is 1.5 times camera 1's) or by 10 px (it fails in
view 1).  Three correspondences have a NaN pixel.  The disc / ring layout leaves a gap in the depths of
triangulateDepth's unit-ray points, where depth_limit_for() puts the limit of that method.
"""
import numpy as np

from deftri.mapmodel import SE3f, mat_from_quat

KB8_1 = np.array([458.654, 457.296, 367.215, 248.375, -0.02, 0.003, 0.0, 0.0], np.float32)
KB8_2 = np.array([1.5 * 458.654, 1.5 * 457.296, 390.0, 250.0, -0.015, 0.002, 0.0, 0.0], np.float32)
# a small camera for 64 x 64 depth images
KB8_SMALL_1 = np.array([70.0, 70.0, 32.0, 32.0, -0.02, 0.003, 0.0, 0.0], np.float32)
KB8_SMALL_2 = np.array([70.0, 70.0, 50.0, 32.0, -0.015, 0.002, 0.0, 0.0], np.float32)
DEPTH_LIMIT = 0.27
LAYERS = (0.20, 0.25, 0.32)


def _project64(k, pc):
    k = k.astype(np.float64)
    theta = np.arctan2(np.hypot(pc[:, 0], pc[:, 1]), pc[:, 2])
    psi = np.arctan2(pc[:, 1], pc[:, 0])
    r = theta + k[4] * theta ** 3 + k[5] * theta ** 5 + k[6] * theta ** 7 + k[7] * theta ** 9
    return np.stack([k[0] * r * np.cos(psi) + k[2], k[1] * r * np.sin(psi) + k[3]], 1)


def poses():
    q1 = np.array([0.004, -0.003, 0.002, 1.0]); q1 /= np.linalg.norm(q1)
    T1w = SE3f(mat_from_quat(q1).astype(np.float32), np.array([0.003, -0.002, 0.001], np.float32))
    q2 = np.array([-0.006, 0.012, 0.004, 1.0]); q2 /= np.linalg.norm(q2)
    R2 = mat_from_quat(q2).astype(np.float32)
    c2 = np.array([0.07, 0.005, -0.04], np.float32)
    return T1w, SE3f(R2, -(R2 @ c2))


def scene(n=300, seed=0, kb8_1=KB8_1, kb8_2=KB8_2, offsets=True, nans=3):
    """(uv1, uv2 float32 [n, 2], kb8_1, kb8_2, T1w, T2w, info): info["layer"] per correspondence,
    info["world"] the points, info["z1"], info["z2"] their true depths."""
    rng = np.random.default_rng(seed)
    T1w, T2w = poses()
    layer = np.where(np.arange(n) % 5 < 3, 0, np.arange(n) % 5 - 2)           # 60 % / 20 % / 20 %
    z = np.take(LAYERS, layer) + rng.uniform(-0.004, 0.004, n)
    ring = np.arange(n) % 2 == 1
    rad = np.where(ring, rng.uniform(0.27, 0.30, n), rng.uniform(0.0, 0.10, n))    # tan of the off-axis angle
    ang = rng.uniform(0, 2 * np.pi, n)
    pc1 = np.stack([rad * np.cos(ang) * z, rad * np.sin(ang) * z, z], 1)
    R1, t1 = T1w.R.astype(np.float64), T1w.t.astype(np.float64)
    R2, t2 = T2w.R.astype(np.float64), T2w.t.astype(np.float64)
    world = (pc1 - t1) @ R1
    pc2 = world @ R2.T + t2
    uv1 = _project64(kb8_1, pc1) + rng.normal(0, 0.1, (n, 2))
    uv2 = _project64(kb8_2, pc2) + rng.normal(0, 0.1, (n, 2))
    if offsets:
        moved = np.arange(n) % 5 == 4
        moved |= np.arange(n) % 10 == 0                                        # some of the first layer too
        step = np.where(np.arange(n) % 4 < 2, 6.0, 10.0) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
        uv2[:, 1] += np.where(moved, step, 0.0) * float(kb8_2[1]) / float(KB8_2[1])
    uv1, uv2 = uv1.astype(np.float32), uv2.astype(np.float32)
    if nans:
        uv1[np.linspace(7, n - 5, nans).astype(int)] = np.nan
    return uv1, uv2, kb8_1, kb8_2, T1w, T2w, {"layer": layer, "world": world, "z1": pc1[:, 2], "z2": pc2[:, 2]}


def depth_limit_for(method, res64):
    """The depth limit of a method on the scene: DEPTH_LIMIT between the layers for the metric seeds;
    for DepthMeasurement (unit-ray points, depths near 1) the middle of the widest gap of the fp64
    restatement's depths (per correspondence the larger of the two views')."""
    if method != "DepthMeasurement":
        return DEPTH_LIMIT
    z = np.maximum(res64["z1"], res64["z2"])
    z = np.sort(z[np.isfinite(z)])
    k = int(np.argmax(np.diff(z)))
    return float(0.5 * (z[k] + z[k + 1]))


def margins_ok(res64, depth_limit, checks, rel=1e-3):
    """No correspondence of the fp64 restatement decides within `rel` of a threshold: z against 0 and
    depth_limit, the squared reprojection errors against 5.991 (when checked), the cosine against 0 and 1."""
    ok = res64["status"] != 1
    far = lambda v, thr, scale: np.abs(v[ok] - thr) > rel * scale
    good = far(res64["z1"], 0.0, depth_limit) & far(res64["z1"], depth_limit, depth_limit)
    good &= far(res64["z2"], 0.0, depth_limit) & far(res64["z2"], depth_limit, depth_limit)
    if checks:
        good &= far(res64["err1"], 5.991, 5.991) & far(res64["err2"], 5.991, 5.991)
    good &= far(res64["cos_parallax"], 1.0, 1.0) & far(res64["cos_parallax"], 0.0, 1.0)
    return bool(good.all())
