"""The two steps between two frames' keypoints and reconstructPoints, restated in numpy (host references
for the library's entries; written from the reference, not from the library's host loops):

  feature_grid(settings)          the Frame's grid and scale pyramid as a dict of deftri_feature_grid's fields
                                  (Frame.cc:213-250, :65-70), for settings without Camera.k1
  frame_grid(ctx, settings)       the same for any settings: with Camera.k1 the bounds are the undistorted image
                                  corners (Context.image_bounds)
  hamming(desc_a, desc_b)         HammingDistance (Modules/Matching/DescriptorMatching.cc:21-36)
  pos_in_grid / build_grid        Frame::posInGrid (Frame.cc:277-286) and the grid distributeFeatures fills (:204-210)
  features_in_area(...)           Frame::getFeaturesInArea (Frame.cc:288-323)
  search_for_initialization(...)  searchForInitializaion (DescriptorMatching.cc:39-99), the sequential loop
  essential_from_poses(...)       computeEssentialMatrixFromPose(T1w * T2w^-1) (Geometry.cc:239-256)
  epipolar_inliers(..., dtype=)   the mask of MonocularMapInitializer::initialize with Triangulation.checks
                                  (MonocularMapInitializer.cc:93-104, :119-178, :206-223), fp32 or fp64

  unit_rays / compute_essential / epipolar_errors / find_essential_ransac_ref / reconstruct_cameras_ref
                                  the RANSAC with a model per hypothesis (computeE :180-203, :119-178) and
                                  reconstructCameras (:246-279) on unit rays, fp32 or fp64, with numpy's SVD

  search_with_projection_ref / guided_matching_ref / map_point_descriptors_ref
                                  searchWithProjection (DescriptorMatching.cc:164-253), guidedMatching (:101-162) and
                                  Map::updateOrientationAndDescriptor (Map.cc:270-321), fp32 or fp64
  guided_matching(ctx, ...) / search_with_projection(ctx, ...)
                                  the two matchers on a context, setting the frame's map point slots
  search_for_triangulation_ref / fuse_search_ref
                                  searchForTriangulation (DescriptorMatching.cc:255-328) and the search inside fuse
                                  (:361-406), fp32 or fp64
  search_for_triangulation(ctx, kf1, kf2, ...) / fuse(ctx, map, kf, ...)
                                  the two on a context: matches between two KeyFrames' free keypoints, and a list of
                                  map points fused into a KeyFrame (Map.fuse_map_points / add_observation)

The device versions are capi.Context.match_for_initialization, .epipolar_inliers, .find_essential_ransac,
.reconstruct_cameras, .search_with_projection, .guided_matching, .map_point_descriptors, .search_for_triangulation
and .fuse_search.  Quirks kept as they
stand: posInGrid rounds half away from zero to a cell index, so a keypoint in the last half cell on the right
or at the bottom is in no cell and never a candidate; only reference keypoints of octave <= 0 are searched;
best and second start at 255; a tie for best rejects; the matches are not one-to-one; the RANSAC scores the
same E, built from the poses, in every iteration, so its result is one evaluation.
"""
import math

import numpy as np

F = np.float32


def feature_grid(settings):
    """The grid of a Frame built from `settings` (Frame.cc:213-250): bounds 0, 0, Camera.cols, Camera.rows
    (no distortion, :222-227).  Camera.k1 present means OpenCV undistortion of keys and bounds: ValueError."""
    if getattr(settings, "has_distortion", False):
        raise ValueError("Camera.k1 is set: the reference undistorts keypoints and image bounds with OpenCV "
                         "(Frame.cc:228-275), which is not restated")
    return {"cols": int(settings.grid_cols), "rows": int(settings.grid_rows), "min_col": 0.0, "min_row": 0.0,
            "max_col": float(int(settings.cols)), "max_row": float(int(settings.rows)),
            "n_scales": int(settings.n_scales), "scale_factor": float(settings.scale_factor)}


def camera_of(settings, what="frame_grid"):
    """(calib, dist) Frame passes to cv::undistortPoints: Camera.fx, fy, cx, cy as float32 [4] and
    Settings.distortion.  With Camera.k1 set, a Camera.fx or Camera.fy that is 0 or missing raises ValueError: the
    undistortion divides by them."""
    dist = np.asarray(getattr(settings, "distortion", ()), F).reshape(-1)
    calib = np.array([settings.fx, settings.fy, settings.cx, settings.cy], F)
    if len(dist) and (calib[0] == 0 or calib[1] == 0):
        raise ValueError(f"{what}: Camera.k1 is set but Camera.fx or Camera.fy is 0 or missing: the reference's "
                         "undistortion (Frame.cc:228-275) divides by them")
    return calib, dist


def frame_grid(ctx, settings):
    """The grid of a Frame built from `settings` (Frame.cc:213-250), for any settings: the dict feature_grid
    returns, with the bounds of Context.image_bounds — 0, 0, Camera.cols, Camera.rows without Camera.k1, the
    undistorted image corners with it (computeImageBoundaries)."""
    calib, dist = camera_of(settings)
    if not len(dist):
        return feature_grid(settings)
    b = ctx.image_bounds(int(settings.cols), int(settings.rows), calib, dist)
    return {"cols": int(settings.grid_cols), "rows": int(settings.grid_rows), "min_col": float(b[0]), "min_row": float(b[1]),
            "max_col": float(b[2]), "max_row": float(b[3]), "n_scales": int(settings.n_scales),
            "scale_factor": float(settings.scale_factor)}


def scale_factors(grid):
    """vScaleFactor_ (Frame.cc:65-70): a running float product."""
    out = [F(1.0)]
    for _ in range(1, grid["n_scales"]):
        out.append(F(out[-1] * F(grid["scale_factor"])))
    return out


def hamming(desc_a, desc_b):
    """HammingDistance of two 32-byte descriptors (or of rows of two [n, 32] arrays): the bit-twiddling
    popcount of DescriptorMatching.cc:28-33 over eight 32-bit words."""
    a = np.ascontiguousarray(desc_a, np.uint8).reshape(-1, 32).view(np.uint32).astype(np.uint64)
    b = np.ascontiguousarray(desc_b, np.uint8).reshape(-1, 32).view(np.uint32).astype(np.uint64)
    v = a ^ b
    v = v - ((v >> 1) & 0x55555555)
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
    d = ((((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) & 0xFFFFFFFF) >> 24
    d = d.sum(1).astype(np.int64)
    return int(d[0]) if np.ndim(desc_a) == 1 and np.ndim(desc_b) == 1 else d


def _round_half_away(v):
    """C's round() of a float32."""
    v = float(v)
    if not math.isfinite(v):
        return v
    return float(math.floor(v + 0.5)) if v >= 0 else -float(math.floor(-v + 0.5))


def _inverses(grid):
    w = F(F(grid["cols"]) / F(F(grid["max_col"]) - F(grid["min_col"])))
    h = F(F(grid["rows"]) / F(F(grid["max_row"]) - F(grid["min_row"])))
    return w, h


def pos_in_grid(grid, x, y):
    """Frame::posInGrid: (ok, col, row) with col = round((x - minCol) * gridElementWidthInv) in float."""
    w, h = _inverses(grid)
    col = _round_half_away(F(F(F(x) - F(grid["min_col"])) * w))
    row = _round_half_away(F(F(F(y) - F(grid["min_row"])) * h))
    ok = (0 <= col < grid["cols"]) and (0 <= row < grid["rows"])      # NaN compares false
    return ok, (int(col) if ok else 0), (int(row) if ok else 0)


def build_grid(grid, uv):
    """grid_[col][row] of Frame::distributeFeatures (Frame.cc:204-210): a keypoint is stored only where its
    own posInGrid is true."""
    cells = [[[] for _ in range(grid["rows"])] for _ in range(grid["cols"])]
    for i, (x, y) in enumerate(np.asarray(uv, F).reshape(-1, 2)):
        ok, c, r = pos_in_grid(grid, x, y)
        if ok:
            cells[c][r].append(i)
    return cells


def features_in_area(grid, cells, uv, octaves, x, y, radius, min_level, max_level):
    """Frame::getFeaturesInArea (Frame.cc:288-323): the indices in visiting order."""
    x, y, radius = F(x), F(y), F(radius)
    ok, min_col, _ = pos_in_grid(grid, F(x - radius), y)
    if not ok:
        min_col = 0
    ok, _, min_row = pos_in_grid(grid, x, F(y - radius))
    if not ok:
        min_row = 0
    ok, max_col, _ = pos_in_grid(grid, F(x + radius), y)
    if not ok:
        max_col = grid["cols"] - 1
    ok, _, max_row = pos_in_grid(grid, x, F(y + radius))
    if not ok:
        max_row = grid["rows"] - 1
    out = []
    for c in range(min_col, max_col + 1):
        for r in range(min_row, max_row + 1):
            for key in cells[c][r]:
                if min_level <= octaves[key] <= max_level:
                    px, py = F(uv[key, 0] - x), F(uv[key, 1] - y)
                    if abs(px) < radius and abs(py) < radius:
                        out.append(key)
    return out


def accept(best, second, th):
    """DescriptorMatching.cc:92: bestDist <= th && (float)bestDist < (float(secondBestDist) * 0.9), the
    product in double."""
    return bool(best <= th and float(F(best)) < float(F(second)) * 0.9)


def search_for_initialization(grid, uv1, octave1, desc1, uv2, octave2, desc2, th, window_size_factor):
    """searchForInitializaion(refFrame = 1, currFrame = 2, th, windowSizeFactor, vMatches), sequentially.
    Returns (matches int32 [n1], best_dist int32 [n1], second_dist int32 [n1], n_matches); the distances are
    255 where a keypoint has no candidate or is not searched."""
    uv1 = np.asarray(uv1, F).reshape(-1, 2); uv2 = np.asarray(uv2, F).reshape(-1, 2)
    octave1 = np.asarray(octave1, np.int64); octave2 = np.asarray(octave2, np.int64)
    desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
    desc2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
    n1 = len(uv1)
    scale = scale_factors(grid)
    cells = build_grid(grid, uv2)
    matches = np.full(n1, -1, np.int32)
    best_d = np.full(n1, 255, np.int32); second_d = np.full(n1, 255, np.int32)
    n_matches = 0
    for i in range(n1):
        if octave1[i] > 0:                                   # only the finest scale (:56)
            continue
        last_octave = int(octave1[i])
        radius = F(F(F(window_size_factor) * 1) * scale[last_octave])
        cand = features_in_area(grid, cells, uv2, octave2, uv1[i, 0], uv1[i, 1], radius, last_octave - 1, last_octave + 1)
        best, second, best_idx = 255, 255, -1
        if cand:
            dist = hamming(np.repeat(desc1[i][None], len(cand), 0), desc2[cand])
            for j, d in zip(cand, dist):
                d = int(d)
                if d < best:
                    second, best, best_idx = best, d, j
                elif d < second:
                    second = d
        if accept(best, second, th):
            matches[i] = best_idx
            n_matches += 1
        best_d[i], second_d[i] = best, second
    return matches, best_d, second_d, n_matches


def essential_from_poses(T1w, T2w, dtype=np.float32):
    """E = [t]x R of T12 = T1w * T2w.inverse() (MonocularMapInitializer.cc:160-163, Geometry.cc:239-256)."""
    dt = np.dtype(dtype).type
    R1, t1, R2, t2 = (np.asarray(a, np.float32).astype(dt) for a in (T1w.R, T1w.t, T2w.R, T2w.t))
    R2i = R2.T
    t2i = -(R2i @ t2)
    R = R1 @ R2i
    t = R1 @ t2i + t1
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], dt)
    return (tx @ R).astype(dt)


def _eigen_normalized(v):
    """Eigen's rowwise normalized(): a row whose squared norm is not positive stays as it is."""
    z = (v * v).sum(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(z > 0, v / np.sqrt(z), v)


def epipolar_inliers(uv1, uv2, kb8_1, kb8_2, T1w, T2w, epipolar_th, dtype=np.float32):
    """computeScoreAndInliers (MonocularMapInitializer.cc:206-223) under the E of the poses — all that
    findEssentialWithRANSAC's 16 identical iterations amount to — for matched pixel pairs, in `dtype`.
    Returns (inlier bool [n], err [n], score)."""
    from .mapping import _kb8_unproject
    dt = np.dtype(dtype)
    uv1 = np.asarray(uv1, F).reshape(-1, 2); uv2 = np.asarray(uv2, F).reshape(-1, 2)
    E = essential_from_poses(T1w, T2w, dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        r1 = _kb8_unproject(kb8_1, uv1, dt); r2 = _kb8_unproject(kb8_2, uv2, dt)
        r1 = r1 / np.linalg.norm(r1, axis=1, keepdims=True)          # :79-80
        r2 = r2 / np.linalg.norm(r2, axis=1, keepdims=True)
        r1_hat = _eigen_normalized((r1 @ E.T).astype(dt))
        d = (r1_hat * _eigen_normalized(r2)).sum(1).astype(dt)
        half_pi = dt.type(np.pi / 2)
        err = np.abs(half_pi - np.arccos(d)).astype(dt)
        inl = err < dt.type(F(epipolar_th))
    return inl, err, int(inl.sum())


# ---- E from the matches alone: computeE per hypothesis, the score of every hypothesis, reconstructCameras ------
def unit_rays(kb8, uv, dtype=np.float64):
    """unproject(uv).normalized() (MonocularMapInitializer.cc:79-80) for rows of uv, in `dtype`."""
    from .mapping import _kb8_unproject
    dt = np.dtype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = _kb8_unproject(kb8, np.asarray(uv, F).reshape(-1, 2), dt).astype(dt)
        return (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(dt)


def _largest_positive(v):
    """v with the sign that makes its component of largest magnitude positive (the lowest index on ties)."""
    return -v if v[int(np.argmax(np.abs(v)))] < 0 else v


def compute_essential(r1, r2, dtype=np.float64):
    """computeE (MonocularMapInitializer.cc:180-203) of eight ray pairs r1, r2 [8, 3] in `dtype`, with numpy's SVD:
    A's row i = [r1_i * r2_i.x, r1_i * r2_i.y, r1_i * r2_i.z]; e = the right singular vector of the smallest singular
    value, its component of largest magnitude positive (the library's choice of the sign an SVD leaves open), as a
    3 x 3; Ef = U diag(1, 1, 0) V^T of e; returns -Ef.  None for a degenerate sample: a ray that is not finite, A of
    rank below 8, or a zero second singular value of e."""
    dt = np.dtype(dtype)
    r1 = np.asarray(r1, dt).reshape(8, 3); r2 = np.asarray(r2, dt).reshape(8, 3)
    if not (np.isfinite(r1).all() and np.isfinite(r2).all()):
        return None
    A = np.concatenate([r1 * r2[:, 0:1], r1 * r2[:, 1:2], r1 * r2[:, 2:3]], 1)
    _, s, Vt = np.linalg.svd(A)
    if not s[7] > 0:
        return None
    e = _largest_positive(Vt[8]).reshape(3, 3)
    U, s3, Vt3 = np.linalg.svd(e)
    if not s3[1] > 0:
        return None
    return (-(U @ np.diag(np.array([1, 1, 0], dt)) @ Vt3)).astype(dt)


def sample_condition(r1, r2):
    """sigma_1 / sigma_8 of a sample's A (fp64): how far an error of the rays is amplified in its null vector."""
    r1 = np.asarray(r1, np.float64).reshape(8, 3); r2 = np.asarray(r2, np.float64).reshape(8, 3)
    s = np.linalg.svd(np.concatenate([r1 * r2[:, 0:1], r1 * r2[:, 1:2], r1 * r2[:, 2:3]], 1), compute_uv=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(s[0] / s[7])


def epipolar_errors(E, r1, r2, dtype=np.float64):
    """computeScoreAndInliers' error (:207-211) of every ray pair under E, in `dtype`: |pi/2 - acos((E r1).normalized()
    . r2.normalized())|, the sums in the order written."""
    dt = np.dtype(dtype)
    E = np.asarray(E, dt).reshape(3, 3); r1 = np.asarray(r1, dt); r2 = np.asarray(r2, dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        Er = np.stack([(E[a, 0] * r1[:, 0] + E[a, 1] * r1[:, 1]) + E[a, 2] * r1[:, 2] for a in range(3)], 1)
        a, b = _eigen_normalized(Er), _eigen_normalized(r2)
        d = ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(dt)
        return np.abs(dt.type(np.pi / 2) - np.arccos(d)).astype(dt)


def find_essential_ransac_ref(r1, r2, samples, epipolar_th, dtype=np.float64, E_all=None):
    """findEssentialWithRANSAC (:119-178) with computeE in every iteration, on unit rays r1, r2 [n, 3] and samples
    [n_hyp, 8], in `dtype`.  E_all [n_hyp, 3, 3] replaces the models (the scores of given models; a zero model counts
    as degenerate).  A degenerate hypothesis (a repeated index, or compute_essential's None) scores 0.  The best is
    replaced on score > bestScore from 0 (:167).  Returns a dict: E, best (-1: every score 0), inlier, err (NaN
    without a best), scores, E_all, degenerate, err_all [n_hyp, n]."""
    dt = np.dtype(dtype)
    r1 = np.asarray(r1, dt); r2 = np.asarray(r2, dt)
    samples = np.asarray(samples, np.int64).reshape(-1, 8)
    H, n = len(samples), len(r1)
    if samples.min() < 0 or samples.max() >= n:
        raise ValueError("a sample index outside [0, n)")
    models = np.zeros((H, 3, 3), dt); deg = np.zeros(H, bool)
    scores = np.zeros(H, np.int64); err_all = np.full((H, n), np.nan, dt)
    th = dt.type(F(epipolar_th))
    best, best_score = -1, 0
    for h in range(H):
        if E_all is not None:
            E = np.asarray(E_all[h], dt).reshape(3, 3)
            E = None if not E.any() else E
        else:
            E = None if len(set(samples[h].tolist())) < 8 else compute_essential(r1[samples[h]], r2[samples[h]], dt)
        if E is None:
            deg[h] = True
            continue
        models[h] = E
        err_all[h] = epipolar_errors(E, r1, r2, dt)
        with np.errstate(invalid="ignore"):
            scores[h] = int((err_all[h] < th).sum())
        if scores[h] > best_score:
            best, best_score = h, int(scores[h])
    with np.errstate(invalid="ignore"):
        inl = err_all[best] < th if best >= 0 else np.zeros(n, bool)
    return {"E": models[best] if best >= 0 else np.zeros((3, 3), dt), "best": best, "inlier": inl,
            "err": err_all[best] if best >= 0 else np.full(n, np.nan, dt), "scores": scores, "E_all": models,
            "degenerate": deg, "err_all": err_all}


def reconstruct_cameras_ref(E, r1, r2, use=None, dtype=np.float64, flip_t0=False):
    """reconstructCameras (:246-262) over decomposeE (:264-279) on unit rays, in `dtype`, with numpy's SVD: R1 = U W^T
    V^T, R2 = U W V^T, each negated when its determinant is negative; Rgood = R2 if trace(R2) > trace(R1) else R1; t =
    U.col(2) with its component of largest magnitude positive (the library's choice; flip_t0 starts from the other
    sign); away = sum of sign((Rgood r1 - r2) . (r2 - t)) over the used rows; t negated when away < 0.  Returns
    (Rgood, t, away)."""
    dt = np.dtype(dtype)
    E = np.asarray(E, dt).reshape(3, 3); r1 = np.asarray(r1, dt); r2 = np.asarray(r2, dt)
    if use is not None:
        use = np.asarray(use, bool)
        r1, r2 = r1[use], r2[use]
    U, _, Vt = np.linalg.svd(E)
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dt)
    R1 = U @ W.T @ Vt
    R2 = U @ W @ Vt
    R1 = -R1 if np.linalg.det(R1) < 0 else R1
    R2 = -R2 if np.linalg.det(R2) < 0 else R2
    Rg = R2 if np.trace(R2) > np.trace(R1) else R1
    t = _largest_positive(U[:, 2] / np.linalg.norm(U[:, 2])).astype(dt)
    if flip_t0:
        t = -t
    with np.errstate(invalid="ignore"):
        a = np.stack([(Rg[i, 0] * r1[:, 0] + Rg[i, 1] * r1[:, 1]) + Rg[i, 2] * r1[:, 2] for i in range(3)], 1) - r2
        b = r2 - t
        s = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        away = int((s > 0).sum()) - int((s < 0).sum())
    return Rg.astype(dt), (-t if away < 0 else t).astype(dt), away


# ---- map points into a frame by projection: guidedMatching, searchWithProjection and what they read ------------
# status of a point (deftri.h): 0 matched, 1 viewCos < 0.5, 2 outside the invariance distances, 3 no candidate,
# 4 candidates but no accepted best, 5 undefined in the reference, 6 a reference slot without a map point
MATCHED, VIEW_COS, INV_DIST, NO_CANDIDATES, REJECTED, UNDEFINED, EMPTY_SLOT = range(7)


def _pose_arrays(Tcw, dt):
    """(R [3, 3], t [3]) in dt of an SE3f or a [3, 4] matrix."""
    if hasattr(Tcw, "R"):
        return np.asarray(Tcw.R, F).astype(dt), np.asarray(Tcw.t, F).astype(dt)
    T = np.asarray(Tcw, F).reshape(3, 4).astype(dt)
    return T[:, :3].copy(), T[:, 3].copy()


def _camera_centre(R, t):
    """Tcw.inverse().translation() = -(R^T t), the sum in the order written."""
    return np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)], R.dtype)


def _to_camera(R, t, X):
    """Tcw * X = R X + t for rows of X, the sums in the order written."""
    return np.stack([((R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1]) + R[i, 2] * X[:, 2]) + t[i] for i in range(3)], 1)


def _project_points(Tcw, kb8, X, dt):
    from .mapping import _kb8_project
    R, t = _pose_arrays(Tcw, dt)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return _kb8_project(kb8, _to_camera(R, t, X.astype(dt)), dt).astype(dt)


def _window_search(grid, cells, uv2, octave2, desc2, slot, i, x, y, radius, octave, desc_i, th):
    """The part guidedMatching (:129-158) and searchWithProjection (:216-249) share for point i: the window,
    the skip of occupied slots, best and second, the acceptance and the claim.  Returns (match, status, best,
    second)."""
    cand = features_in_area(grid, cells, uv2, octave2, x, y, radius, octave - 1, octave + 1)
    if not cand:
        return -1, NO_CANDIDATES, 255, 255
    best, second, best_idx = 255, 255, -1
    dist = hamming(np.repeat(desc_i[None], len(cand), 0), desc2[cand])
    for j, d in zip(cand, dist):
        if slot[j] != -1:                                    # getMapPoint(j): skipped entirely
            continue
        d = int(d)
        if d < best:
            second, best, best_idx = best, d, j
        elif d < second:
            second = d
    if accept(best, second, th):
        slot[best_idx] = i
        return best_idx, MATCHED, best, second
    return -1, REJECTED, best, second


def _frame(uv2, octave2, desc2):
    return (np.asarray(uv2, F).reshape(-1, 2), np.asarray(octave2, np.int64).reshape(-1),
            np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32))


def _report(status):
    return {"n_points": len(status), "n_matches": int((status == MATCHED).sum()), "n_view_cos": int((status == VIEW_COS).sum()),
            "n_inv_dist": int((status == INV_DIST).sum()), "n_no_candidates": int((status == NO_CANDIDATES).sum()),
            "n_rejected": int((status == REJECTED).sum()), "n_undefined": int((status == UNDEFINED).sum())}


def search_with_projection_ref(grid, Tcw, kb8, uv2, octave2, desc2, slot_point, pos, normal, min_dist, max_dist, desc, th,
                               dtype=np.float32):
    """searchWithProjection(currFrame, th, vMapPoints) (DescriptorMatching.cc:164-253), the sequential loop, with
    the float arithmetic in `dtype` (float32 as the reference, or float64).  slot_point [n2]: -1 free, anything
    else occupied.  Returns a dict: match, status, uv, view_cos, predicted_octave, best, second, slot_point,
    report, and the values the decisions were taken on: dist, ratio (log(max / dist) / log(getScaleFactor(1))
    before ceil) and radius."""
    dt = np.dtype(dtype).type
    uv2, octave2, desc2 = _frame(uv2, octave2, desc2)
    X = np.asarray(pos, F).reshape(-1, 3).astype(dt)
    nrm = np.asarray(normal, F).reshape(-1, 3).astype(dt)
    mn, mx = np.asarray(min_dist, F).reshape(-1).astype(dt), np.asarray(max_dist, F).reshape(-1).astype(dt)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n, n_scales = len(X), grid["n_scales"]
    scale = scale_factors(grid)
    slot = np.asarray(slot_point, np.int32).copy()
    cells = build_grid(grid, uv2)
    R, t = _pose_arrays(Tcw, dt)
    centre = _camera_centre(R, t)
    uv = _project_points(Tcw, kb8, X, dt)
    out = {"match": np.full(n, -1, np.int32), "status": np.zeros(n, np.uint8), "uv": uv, "view_cos": np.zeros(n, dt),
           "predicted_octave": np.full(n, -1, np.int32), "best": np.full(n, 255, np.int32), "second": np.full(n, 255, np.int32),
           "dist": np.zeros(n, dt), "ratio": np.full(n, np.nan, dt), "radius": np.zeros(n, dt)}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        log_scale1 = np.log(dt(scale[1]))
        for i in range(n):
            ray = X[i] - centre                                                     # :177
            z = (ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2]
            rn = ray / np.sqrt(z) if z > 0 else ray
            vc = dt((rn[0] * nrm[i, 0] + rn[1] * nrm[i, 1]) + rn[2] * nrm[i, 2])   # :178
            out["view_cos"][i] = vc
            dist = np.sqrt(z)
            out["dist"][i] = dist
            if vc < 0.5:                                                            # :180
                out["status"][i] = VIEW_COS
                continue
            if dist < mn[i] or dist > mx[i]:                                        # :190
                out["status"][i] = INV_DIST
                continue
            ratio = dt(np.log(dt(mx[i] / dist)) / log_scale1)                       # :196
            out["ratio"][i] = ratio
            c = np.ceil(ratio)
            octave = n_scales if (np.isnan(c) or c > n_scales) else 0 if c < 0 else int(c)   # :197-200
            out["predicted_octave"][i] = octave
            if octave >= n_scales or not np.all(np.isfinite(uv[i])):                # vScaleFactor_[nScales]; posInGrid's int
                out["status"][i] = UNDEFINED
                continue
            radius = dt(float(scale[octave]) * (2.5 if float(vc) > 0.998 else 4.0))   # :206-210, in double
            out["radius"][i] = radius
            out["match"][i], out["status"][i], out["best"][i], out["second"][i] = _window_search(
                grid, cells, uv2, octave2, desc2, slot, i, uv[i, 0], uv[i, 1], radius, octave, desc[i], th)
    out["slot_point"] = slot
    out["report"] = _report(out["status"])
    return out


def guided_matching_ref(grid, Tcw, kb8, uv2, octave2, desc2, has_point, pos, octave1, desc, th, window_size_factor,
                        dtype=np.float32):
    """guidedMatching(refFrame, currFrame, th, vMatches, windowSizeFactor) (DescriptorMatching.cc:101-162), the
    sequential loop over the reference frame's slots, the projection in `dtype`.  Returns a dict: match, status, uv,
    best, second, slot_point (the reference slot in each of the current frame's slots, or -1), report, radius."""
    dt = np.dtype(dtype).type
    uv2, octave2, desc2 = _frame(uv2, octave2, desc2)
    has = np.asarray(has_point).reshape(-1).astype(bool)
    X = np.asarray(pos, F).reshape(-1, 3).astype(dt)
    octave1 = np.asarray(octave1, np.int64).reshape(-1)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n1 = len(has)
    scale = scale_factors(grid)
    slot = np.full(len(uv2), -1, np.int32)                                          # clearMapPoints (:102)
    cells = build_grid(grid, uv2)
    uv = _project_points(Tcw, kb8, X, dt)
    uv[~has] = 0
    out = {"match": np.full(n1, -1, np.int32), "status": np.where(has, 0, EMPTY_SLOT).astype(np.uint8), "uv": uv,
           "best": np.full(n1, 255, np.int32), "second": np.full(n1, 255, np.int32), "radius": np.zeros(n1, dt)}
    window15 = 15 * int(window_size_factor)                                         # an int product (:127)
    for i in np.nonzero(has)[0]:
        if not np.all(np.isfinite(uv[i])):
            out["status"][i] = UNDEFINED
            continue
        octave = int(octave1[i])
        radius = F(F(window15) * scale[octave])
        out["radius"][i] = radius
        out["match"][i], out["status"][i], out["best"][i], out["second"][i] = _window_search(
            grid, cells, uv2, octave2, desc2, slot, int(i), uv[i, 0], uv[i, 1], radius, octave, desc[i], th)
    out["slot_point"] = slot
    out["report"] = _report(out["status"])
    return out


def map_point_descriptors_ref(pos, obs_start, obs_kf, obs_slot, kf_Tcw, kf_slot_start, kf_desc, kf_octave, n_scales,
                              scale_factor, dtype=np.float32):
    """Map::updateOrientationAndDescriptor (Map.cc:270-321) for a batch of map points, the observations in the
    order given, the float arithmetic in `dtype`.  Returns a dict: normal, max_dist, min_dist, desc, ref_obs,
    status (1: no observation, nothing written) and medians (per point the list of its observations' medians).
    An ordinal beyond the chosen keyframe's slots raises ValueError."""
    dt = np.dtype(dtype).type
    X = np.asarray(pos, F).reshape(-1, 3).astype(dt)
    T = np.asarray(kf_Tcw, F).reshape(-1, 3, 4).astype(dt)
    kf_desc = np.ascontiguousarray(kf_desc, np.uint8).reshape(-1, 32)
    scale = scale_factors({"n_scales": n_scales, "scale_factor": scale_factor})
    centres = [_camera_centre(Tk[:, :3], Tk[:, 3]) for Tk in T]
    n = len(X)
    out = {"normal": np.zeros((n, 3), dt), "max_dist": np.zeros(n, dt), "min_dist": np.zeros(n, dt),
           "desc": np.zeros((n, 32), np.uint8), "ref_obs": np.full(n, -1, np.int32), "status": np.zeros(n, np.uint8),
           "medians": [[] for _ in range(n)]}

    def normalized(v):
        z = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        return v / np.sqrt(z) if z > 0 else v

    for p in range(n):
        o0, o1 = int(obs_start[p]), int(obs_start[p + 1])
        n_obs = o1 - o0
        if n_obs == 0:
            out["status"][p] = 1
            continue
        kfs = [int(k) for k in obs_kf[o0:o1]]
        rows = [int(kf_slot_start[k]) + int(s) for k, s in zip(kfs, obs_slot[o0:o1])]
        normal = np.zeros(3, dt)
        for k in kfs:                                                               # :286-287
            normal = normal + normalized(X[p] - centres[k])
        normal = normalized(normal / dt(n_obs))                                     # :293
        best_median, obs_idx = F(255.0), 0                                          # :296
        for i in range(n_obs):
            d = np.sort(hamming(np.repeat(kf_desc[rows[i]][None], n_obs, 0), kf_desc[rows]))
            med = int(d[n_obs // 2])                                                # nth_element's element
            out["medians"][p].append(med)
            if med < best_median:
                best_median, obs_idx = F(med), i
        k = kfs[obs_idx]
        if obs_idx >= int(kf_slot_start[k + 1]) - int(kf_slot_start[k]):
            raise ValueError(f"map point {p}: keypoint {obs_idx} (the chosen observation's ordinal, Map.cc:312) is no slot of "
                             f"keyframe {k}")
        ray = X[p] - centres[k]
        dist = np.sqrt((ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2])       # :311
        ref_octave = int(kf_octave[int(kf_slot_start[k]) + obs_idx])                # :312, the ordinal as a slot
        mx = dt(dist * dt(scale[ref_octave]))
        out["normal"][p], out["max_dist"][p], out["min_dist"][p] = normal, mx, dt(mx / dt(scale[n_scales - 1]))
        out["desc"][p] = kf_desc[rows[obs_idx]]
        out["ref_obs"][p] = obs_idx
    return out


def _frame_of(cur_frame, what):
    if getattr(cur_frame, "descriptors", None) is None:
        raise ValueError(f"{what}: the frame has no descriptors")
    return cur_frame.pose, cur_frame.kb8, cur_frame.keypoints, cur_frame.octaves, cur_frame.descriptors


def guided_matching(ctx, ref_frame, cur_frame, grid, th, window_size_factor):
    """guidedMatching(refFrame, currFrame, th, vMatches, windowSizeFactor) on `ctx` (Context.guided_matching): clears
    cur_frame.map_points and sets the matched slots to the reference frame's map points, as the reference sets
    vMapPoints_.  A KeyFrame serves as either frame.  Returns (matches int32 [reference slots], report); a map point
    without a descriptor raises ValueError."""
    frame = _frame_of(cur_frame, "guided_matching")
    n1 = ref_frame.n_slots
    has = np.array([mp is not None for mp in ref_frame.map_points], bool)
    pos = np.zeros((n1, 3), F); desc = np.zeros((n1, 32), np.uint8)
    for i, mp in enumerate(ref_frame.map_points):
        if mp is None:
            continue
        if getattr(mp, "descriptor", None) is None:
            raise ValueError(f"guided_matching: map point {mp.id} has no descriptor (Map.update_orientation_and_descriptor)")
        pos[i], desc[i] = mp.position, mp.descriptor
    res = ctx.guided_matching(grid, *frame, has, pos, ref_frame.octaves, desc, th, window_size_factor)
    cur_frame.map_points = [None if i < 0 else ref_frame.map_points[i] for i in res.slot_point]
    return res.match, res.report


def search_with_projection(ctx, cur_frame, grid, th, map_points):
    """searchWithProjection(currFrame, th, vMapPoints) on `ctx` (Context.search_with_projection): the slots of
    cur_frame.map_points that hold a map point stay as they are, the matched free ones are set.  Returns (matches
    int32 [map points]: the slot or -1, report); a map point without descriptor, normal or invariance distances
    raises ValueError."""
    frame = _frame_of(cur_frame, "search_with_projection")
    map_points = list(map_points)
    for mp in map_points:
        if any(getattr(mp, k, None) is None for k in ("descriptor", "normal", "min_distance", "max_distance")):
            raise ValueError(f"search_with_projection: map point {mp.id} lacks its descriptor, normal or invariance distances "
                             "(Map.update_orientation_and_descriptor)")
    n = len(map_points)
    pos = np.array([mp.position for mp in map_points], F).reshape(n, 3)
    nrm = np.array([mp.normal for mp in map_points], F).reshape(n, 3)
    mn = np.array([mp.min_distance for mp in map_points], F); mx = np.array([mp.max_distance for mp in map_points], F)
    desc = np.array([mp.descriptor for mp in map_points], np.uint8).reshape(n, 32)
    slot = np.array([-1 if mp is None else -2 for mp in cur_frame.map_points], np.int32)
    res = ctx.search_with_projection(grid, *frame, slot, pos, nrm, mn, mx, desc, th)
    for j, i in enumerate(res.slot_point):
        if i >= 0:
            cur_frame.map_points[j] = map_points[i]
    return res.match, res.report


# ---- growing the map past two keyframes: searchForTriangulation and fuse ---------------------------------------
# status of a row of searchForTriangulation (deftri.h): 0 matched, 1 its slot holds a map point, 2 no eligible
# candidate below th, 3 matched and then robbed by a later row, 4 passed over by the vbMatched2[2] quirk
TRI_MATCHED, TRI_OCCUPIED, TRI_NONE, TRI_STOLEN, TRI_FLAG = range(5)


def triangulation_rays(kb8, E, uv1, uv2, dtype=np.float32):
    """ray1 = (E * unproject(uv1)).normalized() (DescriptorMatching.cc:282; the unprojected ray is not normalized first)
    and ray2 = unproject(uv2).normalized() (:300), both with the one calibration (:267), in `dtype`."""
    from .mapping import _kb8_unproject
    dt = np.dtype(dtype)
    E = np.asarray(E, F).reshape(3, 3).astype(dt)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a = _kb8_unproject(kb8, np.asarray(uv1, F).reshape(-1, 2), dt).astype(dt)
        b = _kb8_unproject(kb8, np.asarray(uv2, F).reshape(-1, 2), dt).astype(dt)
        Ea = np.stack([(E[r, 0] * a[:, 0] + E[r, 1] * a[:, 1]) + E[r, 2] * a[:, 2] for r in range(3)], 1).astype(dt)
        return _eigen_normalized(Ea).astype(dt), _eigen_normalized(b).astype(dt)


def triangulation_epipolar_errors(ray1, ray2, dtype=np.float32):
    """float err = fabs(M_PI/2 - acos(ray2.dot(ray1))) (:303) for every pair [n1, n2]: in float32 the dot product and
    acos are float, the difference and fabs double, the result rounded to float; in float64 everything is double."""
    dt = np.dtype(dtype)
    with np.errstate(invalid="ignore"):
        d = ((ray2[None, :, 0] * ray1[:, None, 0] + ray2[None, :, 1] * ray1[:, None, 1]) + ray2[None, :, 2] * ray1[:, None, 2]).astype(dt)
        return np.abs(np.pi / 2 - np.arccos(d).astype(dt).astype(np.float64)).astype(dt)


def search_for_triangulation_ref(uv1, desc1, has_point1, uv2, desc2, has_point2, kb8, E, th, epipolar_th, flag_quirk=True,
                                 dtype=np.float32):
    """searchForTriangulation(kf1, kf2, th, fEpipolarTh, E, vMatches) (DescriptorMatching.cc:255-328), the sequential
    loop, the float arithmetic in `dtype`.  vMatchedDistance and vnMatches21 have n2 elements (the reference sizes them
    by n1 and indexes them by j); vbMatched2 is the one boolean it amounts to (element 2 is all that is read), ignored
    with flag_quirk false.  Returns a dict: matches, best_dist, status, n_matches, report (the counters and flag_row),
    and what the decisions were taken on: dist [n1, n2] and err [n1, n2]."""
    if th > 255:
        raise ValueError("search_for_triangulation: th > 255: the reference would use an uninitialised bestIdx")
    dt = np.dtype(dtype)
    desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); desc2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
    has1 = np.asarray(has_point1).reshape(-1).astype(bool); has2 = np.asarray(has_point2).reshape(-1).astype(bool)
    n1, n2 = len(desc1), len(desc2)
    ray1, ray2 = triangulation_rays(kb8, E, uv1, uv2, dt)
    err = triangulation_epipolar_errors(ray1, ray2, dt)
    bits1 = np.unpackbits(desc1, axis=1).astype(np.int32); bits2 = np.unpackbits(desc2, axis=1).astype(np.int32)
    dist = (bits1.sum(1)[:, None] + bits2.sum(1)[None, :] - 2 * (bits1 @ bits2.T)).astype(np.int64)   # = hamming(), by bits
    with np.errstate(invalid="ignore"):
        passed = err < dt.type(F(epipolar_th))
    matches = np.full(n1, -1, np.int32); best_d = np.full(n1, 255, np.int32)
    status = np.where(has1, TRI_OCCUPIED, TRI_NONE).astype(np.uint8)
    matched_dist = np.full(n2, np.iinfo(np.int32).max, np.int64); match21 = np.full(n2, -1, np.int64)
    flag, flag_row, n_matches = False, -1, 0
    for i in range(n1):
        if has1[i]:                                          # :277
            continue
        if flag_quirk and flag:                              # :288: vbMatched2[2] passes every j over
            status[i] = TRI_FLAG
            continue
        best, best_idx = 255, -1
        for j in np.nonzero(~has2 & (dist[i] <= 50))[0]:     # :288, :293's first half; ascending j
            d = int(dist[i, j])
            if d > best:                                     # :293
                continue
            if matched_dist[j] <= d:                         # :296
                continue
            if passed[i, j]:                                 # :303-307
                best, best_idx = d, int(j)
        if best < th:                                        # :310
            if match21[best_idx] >= 0:                       # :314-317
                matches[match21[best_idx]] = -1
                status[match21[best_idx]] = TRI_STOLEN
                n_matches -= 1
            matches[i], best_d[i], status[i] = best_idx, best, TRI_MATCHED
            match21[best_idx] = i
            if best == 2 and not flag:                       # vbMatched2[bestDist] = true
                flag, flag_row = True, i
            matched_dist[best_idx] = best
            n_matches += 1
    report = {"n1": n1, "n2": n2, "n_matches": n_matches, "n_occupied": int((status == TRI_OCCUPIED).sum()),
              "n_unmatched": int((status == TRI_NONE).sum()), "n_stolen": int((status == TRI_STOLEN).sum()),
              "n_flag_skipped": int((status == TRI_FLAG).sum()), "flag_row": flag_row}
    return {"matches": matches, "best_dist": best_d, "status": status, "n_matches": n_matches, "report": report,
            "dist": dist, "err": err}


def fuse_search_ref(grid, Tcw, kb8, uv2, octave2, desc2, consider, pos, octave, desc, th, dtype=np.float32):
    """The search of fuse (DescriptorMatching.cc:361-406) for every considered point, the projection in `dtype`: no
    depth test, radius = 2.5 * getScaleFactor(octave) in double, levels octave +- 1, no slot is skipped.  Returns a
    dict: match, status, uv, best, second, report, radius."""
    dt = np.dtype(dtype).type
    uv2, octave2, desc2 = _frame(uv2, octave2, desc2)
    con = np.asarray(consider).reshape(-1).astype(bool)
    X = np.asarray(pos, F).reshape(-1, 3).astype(dt)
    octave = np.asarray(octave, np.int64).reshape(-1)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(con)
    scale = scale_factors(grid)
    free = np.full(len(uv2), -1, np.int32)
    cells = build_grid(grid, uv2)
    uv = _project_points(Tcw, kb8, X, dt)
    uv[~con] = 0
    out = {"match": np.full(n, -1, np.int32), "status": np.where(con, 0, EMPTY_SLOT).astype(np.uint8), "uv": uv,
           "best": np.full(n, 255, np.int32), "second": np.full(n, 255, np.int32), "radius": np.zeros(n, dt)}
    for i in np.nonzero(con)[0]:
        if not np.all(np.isfinite(uv[i])):
            out["status"][i] = UNDEFINED
            continue
        o = int(octave[i])
        radius = F(2.5 * float(scale[o]))                                           # :369
        out["radius"][i] = radius
        out["match"][i], out["status"][i], out["best"][i], out["second"][i] = _window_search(
            grid, cells, uv2, octave2, desc2, free.copy(), int(i), uv[i, 0], uv[i, 1], radius, o, desc[i], th)
    out["report"] = _report(out["status"])
    return out


def search_for_triangulation(ctx, kf1, kf2, th, epipolar_th, E=None, flag_quirk=True):
    """searchForTriangulation(kf1, kf2, th, fEpipolarTh, E, vMatches) on `ctx` (Context.search_for_triangulation) for two
    KeyFrames: the keypoints whose slot holds no map point are matched, with kf1's calibration for both (:267).  E
    defaults to essential_from_poses(kf1.pose, kf2.pose), the convention computeScoreAndInliers uses.  flag_quirk
    True is the reference as it stands: after a row accepted at distance exactly 2 no row matches (deftri.h).  Edits
    nothing.  Returns (matches int32 [kf1's slots], report)."""
    for kf in (kf1, kf2):
        if getattr(kf, "descriptors", None) is None:
            raise ValueError(f"search_for_triangulation: keyframe {kf.id} has no descriptors")
    if E is None:
        E = essential_from_poses(kf1.pose, kf2.pose)
    has1 = np.array([mp is not None for mp in kf1.map_points], bool)
    has2 = np.array([mp is not None for mp in kf2.map_points], bool)
    res = ctx.search_for_triangulation(kf1.keypoints, kf1.descriptors, has1, kf2.keypoints, kf2.descriptors, has2, kf1.kb8, E,
                                       th, epipolar_th, flag_quirk)
    return res.matches, res.report


def fuse(ctx, m, kf, th, map_points, grid):
    """fuse(pKF, th, vMapPoints, pMap) (DescriptorMatching.cc:330-428) on `ctx`: one search for all the points that are
    not None (Context.fuse_search; inside fuse a point's search does not depend on earlier iterations), then the
    reference's loop on the host with its three skips evaluated at that moment — the point is null, it has no
    observation (for instance an earlier fusion deleted it), it is already in kf — and for an accepted point
    Map.fuse_map_points with the map point in the matched slot, or Map.add_observation and the slot.  The kept quirk
    of :366: point i is searched at the octave of kf's keypoint i, the list index used as a keypoint index, so a
    list longer than kf's slots raises ValueError.  The descriptors Map::addObservation would refresh per edit are
    refreshed once at the end for the surviving touched points (Map.update_orientation_and_descriptor): a point
    whose descriptor an earlier iteration changed is by then in kf or gone and is skipped, and the final descriptor
    depends only on the final observations and their order.  Returns (n_fused, report)."""
    frame = _frame_of(kf, "fuse")
    map_points = list(map_points)
    n = len(map_points)
    if n > kf.n_slots:
        raise ValueError(f"fuse: {n} map points but keyframe {kf.id} has {kf.n_slots} keypoints: the reference reads "
                         "getKeyPoint(i) of the list index (DescriptorMatching.cc:366)")
    consider = np.array([mp is not None for mp in map_points], bool)
    pos = np.zeros((n, 3), F); desc = np.zeros((n, 32), np.uint8)
    for i, mp in enumerate(map_points):
        if mp is None:
            continue
        if getattr(mp, "descriptor", None) is None:
            raise ValueError(f"fuse: map point {mp.id} has no descriptor (Map.update_orientation_and_descriptor)")
        pos[i], desc[i] = mp.position, mp.descriptor
    res = ctx.fuse_search(grid, *frame, consider, pos, np.asarray(kf.octaves, np.int32)[:n], desc, th)
    n_fused, touched = 0, {}
    for i, mp in enumerate(map_points):
        if mp is None:                                                              # :347
            continue
        if len(m.mp_obs.get(mp.id, {})) == 0:                                       # :350
            continue
        if m.is_map_point_in_keyframe(mp.id, kf.id) != -1:                          # :353
            continue
        if res.status[i] != MATCHED:
            continue
        j = int(res.match[i])
        other = kf.map_points[j]
        if other is not None:                                                       # :411-413
            touched[m.fuse_map_points(mp.id, other.id)] = True
        else:                                                                       # :416-419
            kf.map_points[j] = mp
            m.add_observation(kf.id, mp.id, j)
            touched[mp.id] = True
        n_fused += 1
    alive = [pid for pid in touched if pid in m.map_points and m.mp_obs.get(pid)]
    if alive:
        m.update_orientation_and_descriptor(ctx, alive, grid)
    report = dict(res.report)
    report["n_fused"] = n_fused
    return n_fused, report
