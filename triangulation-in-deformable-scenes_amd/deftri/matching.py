"""The two steps between two frames' keypoints and reconstructPoints, restated in numpy (host references
for the library's entries; written from the reference, not from the library's host loops):

  feature_grid(settings)          the Frame's grid and scale pyramid as a dict of deftri_feature_grid's fields
                                  (Frame.cc:213-250, :65-70)
  hamming(desc_a, desc_b)         HammingDistance (Modules/Matching/DescriptorMatching.cc:21-36)
  pos_in_grid / build_grid        Frame::posInGrid (Frame.cc:277-286) and the grid distributeFeatures fills (:204-210)
  features_in_area(...)           Frame::getFeaturesInArea (Frame.cc:288-323)
  search_for_initialization(...)  searchForInitializaion (DescriptorMatching.cc:39-99), the sequential loop
  essential_from_poses(...)       computeEssentialMatrixFromPose(T1w * T2w^-1) (Geometry.cc:239-256)
  epipolar_inliers(..., dtype=)   the mask of MonocularMapInitializer::initialize with Triangulation.checks
                                  (MonocularMapInitializer.cc:93-104, :119-178, :206-223), fp32 or fp64

The device versions are capi.Context.match_for_initialization and .epipolar_inliers.  Quirks kept as they
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
