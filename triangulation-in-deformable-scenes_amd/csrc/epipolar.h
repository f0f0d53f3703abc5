// epipolar.h — computeScoreAndInliers (MonocularMapInitializer.cc:206-223) for one match, host and device,
// in the reference's float arithmetic (no contraction: the including files are built with
// -ffp-contract=off).  In two parts, so that the RANSAC of essential.hip unprojects a match once and
// scores it under many E: the rays (:79-80), and the error of a ray pair under one E.  matching.hip's
// k_epipolar_inliers and its host loop run the two back to back.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "device_math.h"
#include "matching_grid.h"

namespace deftri {
namespace dev {

struct Kb8 { float k[8]; };
struct Mat3 { float m[9]; };

// refRays_ / currRays_ of one match: unproject(uv).normalized() (:79-80)
__host__ __device__ __forceinline__ void epipolar_rays(const Kb8 &k1, const Kb8 &k2, float u1, float v1, float u2, float v2, V3 &r1,
                                                       V3 &r2) {
    r1 = normalized(kb8_unproject(k1.k, u1, v1));
    r2 = normalized(kb8_unproject(k2.k, u2, v2));
}

// |float(pi/2) - acos((E r1).normalized() . r2n)| with r2n = eigen_normalized(r2), the rowwise().normalized() of :210
__host__ __device__ __forceinline__ float epipolar_score(const float *E, V3 r1, V3 r2n) {
    const V3 Er = v3(E[0] * r1.x + E[1] * r1.y + E[2] * r1.z, E[3] * r1.x + E[4] * r1.y + E[5] * r1.z,
                     E[6] * r1.x + E[7] * r1.y + E[8] * r1.z);
    const V3 r1_hat = eigen_normalized(Er);
    const float d = r1_hat.x * r2n.x + r1_hat.y * r2n.y + r1_hat.z * r2n.z;
    return fabsf((float)(M_PI / 2) - acosf(d));
}

// computeScoreAndInliers (:206-223) for one match: |float(pi/2) - acos(r1_hat . r2.normalized())|
__host__ __device__ __forceinline__ float epipolar_error(const Kb8 &k1, const Kb8 &k2, const Mat3 &E, float u1, float v1, float u2,
                                                         float v2) {
    V3 r1, r2;
    epipolar_rays(k1, k2, u1, v1, u2, v2, r1, r2);
    return epipolar_score(E.m, r1, eigen_normalized(r2));
}

}  // namespace dev
}  // namespace deftri
