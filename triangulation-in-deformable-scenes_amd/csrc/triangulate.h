// triangulate.h — the map-point producers in front of the solver (triangulate.hip): the simulated
// producer for every defined seed, reconstructPoints with its acceptance, and the two keyframes'
// initial depth scales.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/deftri.h"
#include "depth_image.h"

namespace deftri {

// The arguments are those of the C entries, already checked for null pointers by the callers; a
// variant the reference does not define, then a host-only context (device < 0), fail before n == 0
// returns.  The kernels run on `st`.
int triangulate(int device, hipStream_t st, int32_t n, int32_t method, int32_t location, const float *uv1, const float *uv2,
                const float *kb8_1, const float *kb8_2, const float *T1w, const float *T2w, float min_cos, float *x3d_1,
                float *x3d_2, uint8_t *valid, std::string &err);
int reconstruct_points(int device, hipStream_t st, int32_t n, const float *uv1, const float *uv2, const float *kb8_1,
                       const float *kb8_2, const float *T1w, const float *T2w, const deftri_reconstruct_params &params,
                       float *x3d_1, float *x3d_2, uint8_t *status, float *cos_parallax, deftri_reconstruct_report *report,
                       std::string &err);
int init_depth_scales(int device, hipStream_t st, DepthImages &images, int64_t kf_id_1, int64_t kf_id_2, int32_t n,
                      const float *uv1, const float *uv2, const float *x3d_1, const float *x3d_2, const float *kb8_1,
                      const float *kb8_2, const float *T1w, const float *T2w, float min_cos, uint8_t *keep, double *scale_1,
                      double *scale_2, int64_t *n_points, std::string &err);

}  // namespace deftri
