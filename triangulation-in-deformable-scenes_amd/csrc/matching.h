// matching.h — the two steps between two frames' keypoints and reconstructPoints (matching.hip):
// searchForInitializaion (Modules/Matching/DescriptorMatching.cc:39-99) over the current frame's
// feature grid, and the epipolar inlier mask MonocularMapInitializer::initialize builds with
// Triangulation.checks (MonocularMapInitializer.cc:93-104, computeScoreAndInliers :206-223).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/deftri.h"

namespace deftri {

// device < 0: the sequential host loops (a real per-cell grid and the :76-96 loop); else the kernels on
// `st`.  The arguments are those of the C entries, already checked for null pointers by the callers.
int match_for_initialization(int device, hipStream_t st, const deftri_feature_grid &grid, int32_t n1, const float *uv1,
                             const int32_t *octave1, const uint8_t *desc1, int32_t n2, const float *uv2,
                             const int32_t *octave2, const uint8_t *desc2, int32_t th, float window_size_factor,
                             int32_t *matches, int32_t *best_dist, int32_t *second_dist, int32_t *n_matches,
                             std::string &err);
int epipolar_inliers(int device, hipStream_t st, int32_t n, const float *uv1, const float *uv2, const float *kb8_1,
                     const float *kb8_2, const float *T1w, const float *T2w, float epipolar_th, uint8_t *inlier, float *err_out,
                     int32_t *score, std::string &err);
// the current frame's cell lists as the device builds them (Frame::distributeFeatures' grid, Frame.cc:
// 204-210): cell_start [cols * rows + 1], cell c * rows + r holding cell_keys[cell_start[..] ..); the order
// inside a cell is not defined
int feature_grid_cells(int device, hipStream_t st, const deftri_feature_grid &grid, int32_t n, const float *uv,
                       int32_t *cell_start, int32_t *cell_keys, std::string &err);

}  // namespace deftri
