"""The map producer for two real keyframes, Mapping::monocularMapInitialization (Modules/Mapping/
Mapping.cc:131-254): searchForInitializaion and the minMatches gate (:144-156), the epipolar inlier mask of
MonocularMapInitializer::initialize (MonocularMapInitializer.cc:53-112), reconstructPoints (:281-395) and
the map construction with the initial depth scales (Mapping.cc:171-254).

  reconstruct_points()            host restatement of reconstructPoints for matched pixel pairs (fp32 as the
                                  reference, or fp64 for parity bands); the device version is
                                  capi.Context.reconstruct_points (k_reconstruct_points)
  init_depth_scales()             host restatement of the depth filter and estimatedDepthScale_ sums
                                  (Mapping.cc:183-254); the device version is Context.init_depth_scales
  monocular_map_initialization()  the two device steps, then the Map as Mapping.cc:171-254 builds it
  monocular_map_initialization_from_features()
                                  the same from keypoints, octaves and descriptors: the match and the inlier
                                  mask on the device (matching.py holds their host restatements), then
                                  monocular_map_initialization
  compute_max_tries() / ransac_samples() / reconstruct_environment()
                                  the map from two keyframes without a pose for the second: the RANSAC over E with a
                                  model per hypothesis and reconstructCameras on the device (MonocularMapInitializer.cc:
                                  114-279; matching.py holds their host restatements), then monocular_map_initialization
  extract_features()              Mapping::extractFeatures (Mapping.cc:120-129): FAST::extract, then ORB::describe
                                  with the caller's sampling pattern (features.py)
  set_keypoints_from_features()   a keyframe's keypoints, octaves and angles from FAST::extract's result
                                  (features.extract / Context.fast_extract), optionally its descriptors from
                                  ORB::describe's

To monocular_map_initialization and _from_features the poses are inputs, as they are to the reference's RANSAC,
which builds E from them in every iteration (MonocularMapInitializer.cc:160-163); reconstruct_environment
estimates E from the samples (computeE) and the second pose from it (reconstructCameras).  The two matchers the
reference never calls (searchForTriangulation, fuse) are matching.search_for_triangulation and matching.fuse.  Two quirks of the reference are kept as they stand: the current keyframe's
MapPoint goes into slot i, the reference keyframe's index, not vMatches[i] (Mapping.cc:208-209), and
the parallax angle in DEGREES is compared with Triangulation.minCos (:220, and the acceptance test of
reconstructPoints, which receives minCos as fMinParallax, :60).
"""
import math

import numpy as np

from . import matching, sim
from .mapmodel import Map, MapPoint

CHI2_2DOF = 5.991          # the reference's literal (a double)


def _kb8_unproject(kb8, uv, dt):
    """KannalaBrandt8::unproject (KannalaBrandt8.cc:51-83) in dtype dt."""
    if dt == np.float32:
        return sim.kb8_unproject(np.asarray(kb8, np.float32), uv)
    k = np.asarray(kb8, np.float32).astype(dt)
    uv = np.asarray(uv, np.float32).astype(dt)
    px = (uv[:, 0] - k[2]) / k[0]
    py = (uv[:, 1] - k[3]) / k[1]
    theta_d = np.sqrt(px * px + py * py)
    theta = theta_d.copy()
    for _ in range(10):
        t2 = theta * theta; t4 = t2 * t2; t6 = t4 * t2; t8 = t4 * t4
        fix = (theta * (1 + k[4] * t2 + k[5] * t4 + k[6] * t6 + k[7] * t8) - theta_d) / \
              (1 + 3 * k[4] * t2 + 5 * k[5] * t4 + 7 * k[6] * t6 + 9 * k[7] * t8)
        theta = theta - fix
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sin(theta) / theta_d
    return np.stack([s * px, s * py, np.cos(theta)], 1)


def _kb8_project(kb8, pc, dt):
    """KannalaBrandt8::project (KannalaBrandt8.cc:32-49) in dtype dt."""
    if dt == np.float32:
        return sim.kb8_project(np.asarray(kb8, np.float32), pc)
    k = np.asarray(kb8, np.float32).astype(dt)
    theta = np.arctan2(np.sqrt(pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]), pc[:, 2])
    psi = np.arctan2(pc[:, 1], pc[:, 0])
    t2 = theta * theta; t3 = theta * t2; t5 = t3 * t2; t7 = t5 * t2; t9 = t7 * t2
    r = theta + k[4] * t3 + k[5] * t5 + k[6] * t7 + k[7] * t9
    return np.stack([k[0] * r * np.cos(psi) + k[2], k[1] * r * np.sin(psi) + k[3]], 1)


def world_ray_cosine(r1, r2, T1w, T2w, dt=np.float32):
    """cosRayParallax of (T1w.inverse().rotationMatrix() * r1).normalized() and the same for view 2
    (MonocularMapInitializer.cc:324-326, Mapping.cc:214-216)."""
    R1, R2 = np.asarray(T1w.R, dt), np.asarray(T2w.R, dt)
    ray1, ray2 = r1 @ R1, r2 @ R2                       # rows of R^T r
    ray1 = ray1 / np.linalg.norm(ray1, axis=1, keepdims=True)
    ray2 = ray2 / np.linalg.norm(ray2, axis=1, keepdims=True)
    return (ray1 * ray2).sum(1) / (np.linalg.norm(ray1, axis=1) * np.linalg.norm(ray2, axis=1))


def acceptance(status, cos_parallax, min_parallax):
    """reconstructPoints' tail (:370-394) from the per-correspondence status and cosines: the report
    of deftri_reconstruct_points."""
    status = np.asarray(status)
    kept = np.sort(np.asarray(cos_parallax, np.float32)[status == 0])
    rep = {"n_triangulated": 2 * len(kept), "n_nonfinite": int((status == 1).sum()), "n_depth1": int((status == 2).sum()),
           "n_err1": int((status == 3).sum()), "n_depth2": int((status == 4).sum()), "n_err2": int((status == 5).sum()),
           "parallax_deg": 0.0, "accepted": 0}
    if len(kept) == 0:
        return rep
    c = kept[min(50, len(kept) - 1)]
    if c < 0 or c > 1:
        return rep
    degrees = np.float32(float(np.arccos(np.float32(c))) * (180.0 / np.pi))
    rep["parallax_deg"] = float(degrees)
    rep["accepted"] = int(rep["n_triangulated"] >= 25 and degrees > np.float32(min_parallax))
    return rep


def reconstruct_points(uv1, uv2, kb8_1, kb8_2, T1w, T2w, method="NRSLAM", location="FarPoints", depth_limit=0.0,
                       checks=False, min_parallax=0.0, dtype=np.float32):
    """reconstructPoints' loop (:303-367) for matched pixel pairs (uv2 gathered through vMatches_), in
    `dtype`.  Returns a dict: x3d_1, x3d_2 [n,3], status [n] uint8 (0 kept, 1 not finite / isZero, 2
    depth in view 1, 3 reprojection in view 1, 4 depth in view 2, 5 reprojection in view 2; first failure
    wins), cos_parallax [n], report (acceptance()), and the deciding quantities z1, z2, err1, err2."""
    dt = np.dtype(dtype)
    uv1 = np.asarray(uv1, np.float32).reshape(-1, 2); uv2 = np.asarray(uv2, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        r1 = _kb8_unproject(kb8_1, uv1, dt); r2 = _kb8_unproject(kb8_2, uv2, dt)
        r1 = r1 / np.linalg.norm(r1, axis=1, keepdims=True)
        r2 = r2 / np.linalg.norm(r2, axis=1, keepdims=True)
        x1, x2 = sim.triangulate_pair(r1, r2, T1w, T2w, method, location, dtype=dt)
        R1, t1, R2, t2 = (np.asarray(a, dt) for a in (T1w.R, T1w.t, T2w.R, T2w.t))
        c1, c2 = x1 @ R1.T + t1, x2 @ R2.T + t2
        cosp = world_ray_cosine(r1, r2, T1w, T2w, dt)
        e1 = ((uv1.astype(dt) - _kb8_project(kb8_1, c1, dt)) ** 2).sum(1)
        e2 = ((uv2.astype(dt) - _kb8_project(kb8_2, c2, dt)) ** 2).sum(1)
        lim = dt.type(depth_limit)
        bad = ~(np.isfinite(x1).all(1) & np.isfinite(x2).all(1)) | (np.abs(x1) <= 1e-5).all(1) | (np.abs(x2) <= 1e-5).all(1)
        tests = [bad, (c1[:, 2] < 0) | (c1[:, 2] > lim), bool(checks) & (e1.astype(np.float64) > CHI2_2DOF),
                 (c2[:, 2] < 0) | (c2[:, 2] > lim), bool(checks) & (e2.astype(np.float64) > CHI2_2DOF)]
    status = np.zeros(len(uv1), np.uint8)
    for code in (5, 4, 3, 2, 1):                         # the earliest failing test wins
        status[tests[code - 1]] = code
    return {"x3d_1": x1, "x3d_2": x2, "status": status, "cos_parallax": cosp,
            "report": acceptance(status, cosp, min_parallax), "z1": c1[:, 2], "z2": c2[:, 2], "err1": e1, "err2": e2}


def _host_sampler():
    """getDepthMeasure through the library's host function (a host-only context)."""
    from . import capi
    ctx = capi.Context(-1)

    def sample(kf, uv, scaled):
        ctx.set_depth_images([(kf.id, kf.depth_image, kf.image_depth_scale, kf.ph)])
        return ctx.depth_measure(kf.id, uv, scaled)
    return sample


def camera_z_f32(T, x):
    """(T * x).z in float32, one rounding per operation in the order of the device's xform()."""
    R, t = np.asarray(T.R, np.float32), np.asarray(T.t, np.float32)
    x = np.asarray(x, np.float32)
    return ((R[2, 0] * x[:, 0] + R[2, 1] * x[:, 1]) + R[2, 2] * x[:, 2]) + t[2]


def init_depth_scales(kf_ref, kf_cur, uv1, uv2, x3d_1, x3d_2, min_cos, sampler=None):
    """The depth filter and the initial estimatedDepthScale_ of both keyframes (Mapping.cc:183-254) for
    the correspondences reconstructPoints kept, on the host with a sequential fp64 sum.  sampler(kf, uv,
    scaled) -> (depth float64 [n], status uint8 [n]) is getDepthMeasure (default: the library's host
    function).  Returns (keep [n] bool, scale_1, scale_2, n_points); a pixel with a non-zero sampler
    status raises ValueError; n_points == 0 gives NaN scales (the reference's 0 / 0)."""
    sampler = sampler or _host_sampler()
    uv1 = np.asarray(uv1, np.float32).reshape(-1, 2); uv2 = np.asarray(uv2, np.float32).reshape(-1, 2)
    d1, s1 = sampler(kf_ref, uv1, True); d2, s2 = sampler(kf_cur, uv2, True)
    for kf, uv, st in ((kf_ref, uv1, s1), (kf_cur, uv2, s2)):
        if np.any(st):
            i = int(np.flatnonzero(st)[0])
            raise ValueError(f"keyframe {kf.id} correspondence {i}: pixel ({uv[i, 0]:g}, {uv[i, 1]:g}) has depth status {st[i]}")
    d1u, _ = sampler(kf_ref, uv1, False); d2u, _ = sampler(kf_cur, uv2, False)
    inside = lambda uv: ~((uv[:, 0].astype(np.float64) <= 0.1) | (uv[:, 0] >= 1500) | (uv[:, 1].astype(np.float64) <= 0.1) |
                          (uv[:, 1] >= 1500))
    keep = ~((d1 <= 0.0) | (d2 <= 0.0)) & inside(uv1) & inside(uv2)
    with np.errstate(invalid="ignore", divide="ignore"):
        r1 = sim.kb8_unproject(kf_ref.kb8, uv1); r2 = sim.kb8_unproject(kf_cur.kb8, uv2)
        r1 = r1 / np.linalg.norm(r1, axis=1, keepdims=True)
        r2 = r2 / np.linalg.norm(r2, axis=1, keepdims=True)
        cosp = world_ray_cosine(r1, r2, kf_ref.pose, kf_cur.pose).astype(np.float32)
        degrees = (np.arccos(cosp).astype(np.float32).astype(np.float64) * (180.0 / np.pi)).astype(np.float32)
    use = keep & (degrees > np.float32(min_cos))          # degrees against minCos, as the reference (:220)
    z1 = camera_z_f32(kf_ref.pose, x3d_1).astype(np.float64)
    z2 = camera_z_f32(kf_cur.pose, x3d_2).astype(np.float64)
    scale1 = scale2 = 0.0
    n_points = 0
    for i in np.flatnonzero(use):
        scale1 += d1u[i] / z1[i]
        scale2 += d2u[i] / z2[i]
        n_points += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        scale1, scale2 = np.float64(scale1) / np.float64(n_points), np.float64(scale2) / np.float64(n_points)
    return keep, float(scale1), float(scale2), n_points


def monocular_map_initialization(ctx, kf_ref, kf_cur, matches, settings):
    """Two real keyframes (poses, keypoints, depth images) and vMatches (matches[i] = the current
    keyframe's keypoint matched to the reference keyframe's keypoint i, < 0 for none) to the Map
    arapOptimization expects, as Mapping.cc:171-254: reconstructPoints and the depth-scale step on the
    device of `ctx`, then both keyframes inserted, one MapPoint pair per kept correspondence with the
    observations (ref, i) and (cur, matches[i]), both slots at index i (the reference's slot quirk,
    :208-209), and estimated_depth_scale on both keyframes.  Settings: trian_method, trian_location,
    depth_limit, trian_checks, min_cos (also reconstructPoints' fMinParallax, Mapping.cc:60).
    Returns (Map, report); the Map is None when reconstructPoints does not accept the pair (:164-166)."""
    matches = np.asarray(matches, np.int64)
    idx = np.flatnonzero(matches >= 0)
    uv1 = np.ascontiguousarray(kf_ref.keypoints[idx], np.float32)
    uv2 = np.ascontiguousarray(kf_cur.keypoints[matches[idx]], np.float32)
    x1, x2, status, _cosp, report = ctx.reconstruct_points(
        uv1, uv2, kf_ref.kb8, kf_cur.kb8, kf_ref.pose, kf_cur.pose, method=settings.trian_method,
        location=settings.trian_location, depth_limit=settings.depth_limit, checks=settings.trian_checks,
        min_parallax=settings.min_cos)
    if not report["accepted"]:
        return None, report
    m = Map()
    m.insert_keyframe(kf_ref)
    m.insert_keyframe(kf_cur)
    ctx.register_depth_images(m)
    tri = np.flatnonzero(status == 0)
    keep, scale1, scale2, n_points = ctx.init_depth_scales(kf_ref.id, kf_cur.id, uv1[tri], uv2[tri], x1[tri], x2[tri],
                                                           kf_ref.kb8, kf_cur.kb8, kf_ref.pose, kf_cur.pose, settings.min_cos)
    next_id = 0
    for k in tri[keep]:
        i = int(idx[k])
        mp1, mp2 = MapPoint(x1[k], next_id), MapPoint(x2[k], next_id + 1)
        next_id += 2
        m.insert_map_point(mp1); m.insert_map_point(mp2)
        m.add_observation(kf_ref.id, mp1.id, i)
        m.add_observation(kf_cur.id, mp2.id, int(matches[i]))
        kf_ref.map_points[i] = mp1
        kf_cur.map_points[i] = mp2
    kf_ref.estimated_depth_scale = scale1
    kf_cur.estimated_depth_scale = scale2
    report = dict(report, n_scale_points=n_points, n_map_points=next_id)
    return m, report


def monocular_map_initialization_from_features(ctx, kf_ref, kf_cur, settings):
    """Mapping::monocularMapInitialization (Mapping.cc:131-254) from two keyframes' keypoints, octaves and
    descriptors (KeyFrame.descriptors, uint8 [n, 32]), poses and depth images, on the device of `ctx`:
      searchForInitializaion(ref, cur, Matching.initialization, Matching.initialization.radius) (:144);
      fewer than Triangulation.minMatches matches: (None, report) (:151-156);
      with Triangulation.checks the epipolar inlier mask under Epipolar.th (MonocularMapInitializer.cc:93-104)
      — fewer than 8 matches raise, as cv::kmeans does there; a score of 0 leaves nothing to triangulate:
      (None, report);
      then monocular_map_initialization on the surviving matches.
    The grid is matching.frame_grid's: with Camera.k1 its bounds are the undistorted image corners, and the
    keyframes' keypoints are expected undistorted (set_keypoints_from_features with distribute's result).  Camera.k1
    with a Camera.fx or Camera.fy that is 0 or missing raises ValueError before the context is touched.
    report["n_matches"] is the match count; with checks report["n_inliers"] the score."""
    grid = matching.frame_grid(ctx, settings)
    if kf_ref.descriptors is None or kf_cur.descriptors is None:
        raise ValueError("both keyframes need descriptors")
    matches, _best, _second, n_matches = ctx.match_for_initialization(
        grid, kf_ref.keypoints, kf_ref.octaves, kf_ref.descriptors, kf_cur.keypoints, kf_cur.octaves, kf_cur.descriptors,
        settings.matching_init_th, settings.matching_init_radius)
    report = {"n_matches": n_matches, "accepted": 0}
    if n_matches < np.float32(settings.min_matches):          # :151, getMinMatches() is a float
        return None, report
    matches = matches.astype(np.int64)
    if settings.trian_checks:
        idx = np.flatnonzero(matches >= 0)
        inlier, _err, score = ctx.epipolar_inliers(kf_ref.keypoints[idx], kf_cur.keypoints[matches[idx]], kf_ref.kb8,
                                                   kf_cur.kb8, kf_ref.pose, kf_cur.pose, settings.epipolar_th)
        report["n_inliers"] = score
        if score == 0:                                        # vBestInliers stays empty: nTriangulated == 0
            return None, report
        matches[idx[~inlier]] = -1
    m, rep = monocular_map_initialization(ctx, kf_ref, kf_cur, matches, settings)
    return m, dict(rep, **{k: v for k, v in report.items() if k != "accepted"})


def compute_max_tries(inlier_fraction, success_likelihood):
    """computeMaxTries (MonocularMapInitializer.cc:114-117): log(1 - p) / log(1 - w^8) of two floats, truncated;
    (0.8, 0.95), the reference's arguments (:140), gives 16."""
    w, p = float(np.float32(inlier_fraction)), np.float32(success_likelihood)
    return int(math.log(float(np.float32(1) - p)) / math.log(1.0 - w ** 8))


def ransac_samples(uv1, n_hyp, seed=10, return_labels=False):
    """Samples for Context.find_essential_ransac in the shape of MonocularMapInitializer.cc:128-155, not its draws:
    the reference keypoints uv1 [n, 2] in eight spatial clusters (Lloyd iterations from eight seeded picks, ten
    rounds; an empty cluster takes the point farthest from its centre out of a cluster that has more than one), and per
    hypothesis one index drawn from each cluster, in cluster order.  The reference clusters with cv::kmeans under
    OpenCV's RNG and draws with random_shuffle under srand(10); neither sequence is reproduced.  Returns int32
    [n_hyp, 8] (and the labels int [n] with return_labels).  Fewer than 8 points raise ValueError, as cv::kmeans
    refuses them."""
    uv = np.asarray(uv1, np.float64).reshape(-1, 2)
    n = len(uv)
    if n < 8:
        raise ValueError(f"ransac_samples: {n} points for 8 clusters")
    rng = np.random.default_rng(seed)
    centres = uv[rng.choice(n, 8, replace=False)].copy()
    labels = np.zeros(n, np.int64)
    for _ in range(10):
        d = ((uv[:, None, :] - centres[None]) ** 2).sum(2)
        labels = np.argmin(np.where(np.isnan(d), np.inf, d), 1)
        for c in range(8):
            if (labels == c).any():
                centres[c] = np.nanmean(uv[labels == c], 0) if np.isfinite(uv[labels == c]).all(1).any() else centres[c]
    for c in range(8):
        if not (labels == c).any():
            size = np.bincount(labels, minlength=8)
            d = ((uv - centres[labels]) ** 2).sum(1)
            d = np.where(np.isnan(d), -1.0, d)
            d[size[labels] < 2] = -2.0
            k = int(np.argmax(d))
            labels[k] = c
            centres[c] = uv[k]
    clusters = [np.flatnonzero(labels == c) for c in range(8)]
    samples = np.stack([[cl[rng.integers(len(cl))] for cl in clusters] for _ in range(int(n_hyp))]).astype(np.int32)
    return (samples, labels) if return_labels else samples


def reconstruct_environment(ctx, kf_ref, kf_cur, matches, settings, samples=None, n_hypotheses=None, seed=10):
    """reconstructEnvironment (MonocularMapInitializer.cc:225-244) behind findEssentialWithRANSAC with a model per
    hypothesis (:119-203), for two keyframes of which only the reference has a pose, on the device of `ctx`:
      the RANSAC over the matched pixel pairs (Context.find_essential_ransac) with `samples` [n_hyp, 8], indices into
      the matched pairs in the order of the reference keypoints (default: ransac_samples of n_hypotheses, by default
      computeMaxTries(0.8, 0.95) = 16, under `seed`); its inliers are vTriangulated;
      reconstructCameras on the inliers (Context.reconstruct_cameras): kf_cur.pose = (Rgood, t), kf_ref's pose is
      passed through as the reference passes T1w;
      monocular_map_initialization on the matches masked to the inliers.
    Returns (Map, report): report["n_inliers"] the best score, ["best"], ["n_hypotheses"], ["n_degenerate"], ["away"]
    next to monocular_map_initialization's.  The Map is None and kf_cur.pose is restored when every score is 0 or
    reconstructPoints does not accept the pair.  Fewer than 8 matches raise, as cv::kmeans does in the reference.
    The keypoints are the keyframes' undistorted ones; Camera.k1 with a Camera.fx or Camera.fy that is 0 or missing
    raises ValueError before the context is touched, as it does for matching.frame_grid."""
    matching.camera_of(settings, "reconstruct_environment")
    matches = np.asarray(matches, np.int64).copy()
    idx = np.flatnonzero(matches >= 0)
    uv1 = np.ascontiguousarray(kf_ref.keypoints[idx], np.float32)
    uv2 = np.ascontiguousarray(kf_cur.keypoints[matches[idx]], np.float32)
    if samples is None:
        samples = ransac_samples(uv1, compute_max_tries(0.8, 0.95) if n_hypotheses is None else n_hypotheses, seed)
    res = ctx.find_essential_ransac(uv1, uv2, kf_ref.kb8, kf_cur.kb8, samples, settings.epipolar_th)
    report = {"n_matches": len(idx), "n_inliers": res.report["best_score"], "best": res.report["best"],
              "n_hypotheses": res.report["n_hypotheses"], "n_degenerate": res.report["n_degenerate"], "accepted": 0}
    if res.report["best"] < 0:                                # vBestInliers stays empty: nothing to triangulate
        return None, report
    matches[idx[~res.inlier]] = -1
    pose, away = ctx.reconstruct_cameras(uv1, uv2, kf_ref.kb8, kf_cur.kb8, res.E, res.inlier)
    report["away"] = away
    old = kf_cur.pose
    kf_cur.pose = pose
    try:
        m, rep = monocular_map_initialization(ctx, kf_ref, kf_cur, matches, settings)
    except Exception:
        kf_cur.pose = old
        raise
    if m is None:
        kf_cur.pose = old
    return m, dict(rep, **{k: v for k, v in report.items() if k != "accepted"})


def extract_features(ctx, image, settings, pattern, border_mask=None, distribute=False, n_slots=None):
    """Mapping::extractFeatures (Mapping.cc:120-129) for one 8-bit grey image on `ctx`: features.extract, then
    features.describe of its (distorted) keypoints with the caller's sampling pattern.  Returns (capi.FastResult,
    capi.OrbResult).  With distribute=True the third line runs too, features.distribute of the keypoints over
    n_slots slots (the frame's capacity; default the keypoints alone), and its capi.DistributedFeatures is the
    third element returned."""
    from . import features
    keys = features.extract(ctx, image, settings, border_mask)
    described = features.describe(ctx, image, keys, settings, pattern)
    if not distribute:
        return keys, described
    return keys, described, features.distribute(ctx, keys, settings, n_slots)


def extract_and_distribute_features(ctx, image, settings, pattern, border_mask=None, n_slots=None):
    """extract_features with its third line: (capi.FastResult, capi.OrbResult, capi.DistributedFeatures)."""
    return extract_features(ctx, image, settings, pattern, border_mask, distribute=True, n_slots=n_slots)


def set_keypoints_from_features(kf, result, described=None, distributed=None):
    """Frame::vKeys_ of a keyframe from FAST::extract's result (a capi.FastResult): keypoints, octaves and
    angles of the first len(result) slots; the slots behind them keep zeros, as the reference's vectors of
    nFeatures elements do.  More keypoints than slots raise ValueError (extract stops at the capacity it is
    given, max_keys).  described: ORB::describe's result for the same keypoints (a capi.OrbResult), which
    also fills KeyFrame.descriptors (uint8 [n_slots, 32], zeros behind the keypoints, as the reference's
    cv::Mat of nFeatures rows); without it the descriptors stay as they are.  distributed: features.distribute's
    result for the same keypoints (a capi.DistributedFeatures over len(result) or kf.n_slots slots): kf.keypoints
    then holds its undistorted keys (vKeys_, what every matcher and the graph build read; over n_slots slots also
    the undistorted zeros behind the keypoints, as in the reference) and kf.keypoints_dis the distorted ones
    (vKeysDis_).  Returns the number of keypoints set."""
    n = len(result)
    if n > kf.n_slots:
        raise ValueError(f"{n} keypoints for a keyframe of {kf.n_slots} slots: pass max_keys = n_slots to the extraction")
    if distributed is not None and len(distributed) not in (n, kf.n_slots):
        raise ValueError(f"undistorted keys of {len(distributed)} slots for {n} keypoints in {kf.n_slots} slots")
    if described is not None:
        if len(described) != n:
            raise ValueError(f"{len(described)} descriptors for {n} keypoints")
        kf.descriptors = np.zeros((kf.n_slots, 32), np.uint8)
        kf.descriptors[:n] = described.desc
    kf.keypoints[:] = 0
    kf.octaves[:] = 0
    kf.angles = np.zeros(kf.n_slots, np.float32)
    kf.keypoints[:n] = result.uv
    kf.octaves[:n] = result.octave
    kf.angles[:n] = result.angle
    if distributed is not None:
        kf.keypoints_dis = kf.keypoints.copy()
        kf.keypoints[:len(distributed)] = distributed.uv
    return n
