// essential.h — the part of MonocularMapInitializer that estimates the second pose (essential.hip):
// findEssentialWithRANSAC with a model per iteration (MonocularMapInitializer.cc:119-178, computeE
// :180-203, computeScoreAndInliers :206-223) and reconstructCameras (:246-279, decomposeE :264-279).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/deftri.h"

namespace deftri {

// device < 0: the sequential host loops of the same functions; else the kernels on `st`.  The arguments
// are those of the C entries, already checked for null pointers and sizes by the callers.
int find_essential_ransac(int device, hipStream_t st, int32_t n, const float *uv1, const float *uv2, const float *kb8_1,
                          const float *kb8_2, int32_t n_hyp, const int32_t *samples, float epipolar_th, float *E_best,
                          uint8_t *inlier, float *err_out, int32_t *scores, float *E_all, uint8_t *degenerate,
                          deftri_essential_report *report, std::string &err);
int reconstruct_cameras(int device, hipStream_t st, int32_t n, const float *uv1, const float *uv2, const float *kb8_1,
                        const float *kb8_2, const uint8_t *use, const float *E, float *T2w, int32_t *away, std::string &err);

}  // namespace deftri
