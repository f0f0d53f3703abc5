// undistort.h — Frame's undistortion and feature distribution (undistort.hip): cv::undistortPoints as
// Frame::undistortKeys and Frame::computeImageBoundaries call it (Frame.cc:221-275), restated from its
// definition, and Frame::distributeFeatures (:190-211) over it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/deftri.h"

namespace deftri {

// K (the float fx, fy, cx, cy) and the float coefficients k1, k2, p1, p2[, k3] widened to double
struct UndistortModel {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

// cv::undistortPoints(src, dst, K, dist, R = empty, P = K) for one point with the default termination (5
// iterations, count only), in double from the float pixel, rounded to float at the end.  One rounding per
// operation: the including files are built without contraction.
__host__ __device__ __forceinline__ void undistort_point(const UndistortModel &M, float u, float v, float &ou, float &ov) {
    const double ifx = 1.0 / M.fx, ify = 1.0 / M.fy;
    const double x0 = ((double)u - M.cx) * ifx, y0 = ((double)v - M.cy) * ify;
    double x = x0, y = y0;
    for (int it = 0; it < 5; it++) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1 + ((M.k3 * r2 + M.k2) * r2 + M.k1) * r2);
        if (icdist < 0) {   // the point is given up: its undistorted position is the distorted one
            x = x0;
            y = y0;
            break;
        }
        const double dX = 2 * M.p1 * x * y + M.p2 * (r2 + 2 * x * x);
        const double dY = M.p1 * (r2 + 2 * y * y) + 2 * M.p2 * x * y;
        x = (x0 - dX) * icdist;
        y = (y0 - dY) * icdist;
    }
    ou = (float)(x * M.fx + M.cx);
    ov = (float)(y * M.fy + M.cy);
}

// device < 0: the sequential host loops; else the kernels on `st`.  The arguments are those of the C entries
// (include/deftri.h), already checked for null pointers and negative sizes by the callers.
int undistort_points(int device, hipStream_t st, int32_t n, const float *uv_in, const float *calib, const float *dist,
                     int32_t n_dist, float *uv_out, std::string &err);
int image_bounds(int32_t cols, int32_t rows, const float *calib, const float *dist, int32_t n_dist, float *bounds,
                 std::string &err);
int distribute_features(int device, hipStream_t st, int32_t grid_cols, int32_t grid_rows, int32_t n_scales, float scale_factor,
                        int32_t cols, int32_t rows, const float *calib, const float *dist, int32_t n_dist, int32_t n,
                        const float *uv_dis, float *uv, deftri_feature_grid *grid, int32_t *cell_start, int32_t *cell_items,
                        uint8_t *in_grid, std::string &err);

}  // namespace deftri
