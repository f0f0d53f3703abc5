// triangulate.hip — the map-point producer in front of the solver, one thread per correspondence
// (SURVEY §8(f) row 4): Mapping::triangulateSimulatedMapPoints (reference
// Modules/Mapping/Mapping.cc:280-349); with the Simulation.yaml settings Triangulation.method
// "NRSLAM" and seed.location "FarPoints" that is k_triangulate<NRSLAM, FarPoints>:
//   xn = normalize(KannalaBrandt8::unproject(uv))            KannalaBrandt8.cc:51-83 (Newton on theta,
//                                                             10 steps, stop at |fix| < 1e-6)
//   triangulateNRSLAM(xn1, xn2, T1w, T2w, "FarPoints")       Geometry.cc:103-153
//   isValidParallax: both depths >= 0, cos(ray1, ray2) <= minCos   Mapping.cc:351-366
// Everything in fp32 without FMA contraction, as the reference's Eigen/Sophus float code.
//
// k_triangulate is that producer for every seed the reference defines (useTriangulationMethod,
// Geometry.cc:216-230): triangulateNRSLAM with TwoPoints / FarPoints / in-rays (:103-153) and
// triangulateClassic with TwoPoints / in-rays (:62-101).  k_reconstruct_points is the real-image
// producer, MonocularMapInitializer::reconstructPoints (MonocularMapInitializer.cc:303-367), which also
// takes triangulateDepth (:189-214) on the unit rays; k_init_depth_scales is the initial
// estimatedDepthScale_ of both keyframes (Mapping.cc:183-254) from the context's depth images.
// Method and location are template parameters: a launch runs one variant, no thread diverges on them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "dev_arena.h"
#include "device_math.h"
#include "pose_host.h"
#include "triangulate.h"

namespace deftri {
namespace dev {

#pragma clang fp contract(off)
// V3 and its arithmetic, kb8_unproject: device_math.h
// T = [R | t] row-major 3x4
__device__ __forceinline__ V3 rot(const float *T, V3 p) {
    return v3(T[0] * p.x + T[1] * p.y + T[2] * p.z, T[4] * p.x + T[5] * p.y + T[6] * p.z,
              T[8] * p.x + T[9] * p.y + T[10] * p.z);
}
__device__ __forceinline__ V3 rotT(const float *T, V3 p) {     // R^T p
    return v3(T[0] * p.x + T[4] * p.y + T[8] * p.z, T[1] * p.x + T[5] * p.y + T[9] * p.z,
              T[2] * p.x + T[6] * p.y + T[10] * p.z);
}
__device__ __forceinline__ V3 xform(const float *T, V3 p) { return add(rot(T, p), v3(T[3], T[7], T[11])); }

// ---- the seeds: p3D1 / p3D2 in camera 2's frame (the callers apply T2w.inverse()) ----------------
// triangulateNRSLAM (Geometry.cc:103-153)
template <int LOC>
__device__ __forceinline__ void tri_nrslam(V3 xn1, V3 xn2, const float *T21, V3 &p3D1, V3 &p3D2) {
    const V3 f0 = normalized(xn1), f1 = normalized(xn2);
    const V3 t = v3(T21[3], T21[7], T21[11]);
    const V3 Rf0 = rot(T21, f0);
    const V3 p = cross(Rf0, f1), q = cross(Rf0, t), r = cross(f1, t);
    const float pn = nrm(p), qn = nrm(q), rn = nrm(r);
    const float lambda0 = rn / pn, lambda1 = qn / pn;
    V3 point0 = scl(lambda0, Rf0);
    const V3 point1 = scl(lambda1, f1);
    const V3 x1 = scl(qn / (qn + rn), add(t, scl(rn / pn, add(Rf0, f1))));
    if (LOC == DEFTRI_LOC_TWOPOINTS) {
        p3D1 = x1;
        p3D2 = x1;
    } else if (LOC == DEFTRI_LOC_FARPOINTS) {
        point0 = add(t, point0);
        p3D1 = add(point0, sub(point0, x1));
        p3D2 = add(point1, sub(point1, x1));
    } else {
        p3D1 = add(t, point0);
        p3D2 = point1;
    }
}

// triangulateClassic (Geometry.cc:62-101).  n = svd.matrixV().col(1) of the 2x3 A = M^T (I - t t^T):
// A t = 0, so col(2) = +-t and col(1) is orthogonal to t and to the major right-singular vector v0.
// v0 = A^T u / |A^T u| with u the major eigenvector of the symmetric 2x2 A A^T, n = t x v0 (its sign
// cancels in m - (m.n) n).  No iterative SVD: the fp32 JacobiSVD separates col(1) from the null vector
// only by sigma_1 and loses it.  FarPoints falls into the reference's else branch.
template <int LOC>
__device__ __forceinline__ void tri_classic(V3 xn1, V3 xn2, const float *T21, V3 &p3D1, V3 &p3D2) {
    const V3 m0 = rot(T21, xn1), m1 = xn2;
    const V3 t21 = v3(T21[3], T21[7], T21[11]);
    const V3 t = normalized(t21);
    const V3 c0 = normalized(m0), c1 = normalized(m1);
    const V3 a0 = sub(c0, scl(dot(c0, t), t)), a1 = sub(c1, scl(dot(c1, t), t));     // the rows of A
    const float g00 = dot(a0, a0), g01 = dot(a0, a1), g11 = dot(a1, a1);
    const float hd = 0.5f * (g00 - g11);
    const float lam = 0.5f * (g00 + g11) + sqrtf(hd * hd + g01 * g01);
    // (A A^T - lam I) u = 0: u = (lam - g11, g01) or (g01, lam - g00), the longer of the two
    const bool first = g00 >= g11;
    float ux = first ? lam - g11 : g01, uy = first ? g01 : lam - g00;
    if (ux == 0.0f && uy == 0.0f) ux = 1.0f;                  // A A^T a multiple of I: any u
    const V3 v0 = normalized(add(scl(ux, a0), scl(uy, a1)));
    const V3 n = normalized(cross(t, v0));
    const V3 m0_ = sub(m0, scl(dot(m0, n), n)), m1_ = sub(m1, scl(dot(m1, n), n));
    const V3 z = cross(m1_, m0_);
    const float zz = dot(z, z);
    const float lambda0 = dot(z, cross(t21, m1_)) / zz;
    const float lambda1 = dot(z, cross(t21, m0_)) / zz;
    if (LOC == DEFTRI_LOC_TWOPOINTS) {
        p3D1 = add(t21, scl(lambda0, m0_));
        p3D2 = p3D1;
    } else {
        p3D1 = add(t21, scl(lambda0, m0));
        p3D2 = scl(lambda1, m1);
    }
}

// triangulateDepth (Geometry.cc:189-214): plain arithmetic on the two inputs
template <int LOC>
__device__ __forceinline__ void tri_depth(V3 xn1, V3 xn2, const float *T21, V3 &p3D1, V3 &p3D2) {
    const V3 point0 = xform(T21, xn1), point1 = xn2;
    const V3 s = add(point0, point1);
    const V3 x1 = v3(s.x / 2.0f, s.y / 2.0f, s.z / 2.0f);
    if (LOC == DEFTRI_LOC_TWOPOINTS) {
        p3D1 = x1;
        p3D2 = x1;
    } else if (LOC == DEFTRI_LOC_FARPOINTS) {
        p3D1 = add(point0, sub(point0, x1));
        p3D2 = add(point1, sub(point1, x1));
    } else {
        p3D1 = point0;
        p3D2 = point1;
    }
}

template <int METHOD, int LOC>
__device__ __forceinline__ void tri_seed(V3 xn1, V3 xn2, const float *T21, V3 &p3D1, V3 &p3D2) {
    if (METHOD == DEFTRI_TRI_CLASSIC) tri_classic<LOC>(xn1, xn2, T21, p3D1, p3D2);
    else if (METHOD == DEFTRI_TRI_DEPTH) tri_depth<LOC>(xn1, xn2, T21, p3D1, p3D2);
    else tri_nrslam<LOC>(xn1, xn2, T21, p3D1, p3D2);
}

__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
// cosRayParallax of the two world rays (Geometry.cc:30-32)
__device__ __forceinline__ float cos_world_rays(const float *T1w, const float *T2w, V3 xn1, V3 xn2) {
    const V3 ray1 = normalized(rotT(T1w, xn1)), ray2 = normalized(rotT(T2w, xn2));
    return dot(ray1, ray2) / (nrm(ray1) * nrm(ray2));
}

// Tp: T1w, T2w, T21 = T2w T1w^-1, T2w^-1 (3x4 each, formed on the host as Sophus does)
template <int METHOD, int LOC>
__global__ void k_triangulate(int n, const float *__restrict__ uv1, const float *__restrict__ uv2,
                              const float *__restrict__ kb1, const float *__restrict__ kb2,
                              const float *__restrict__ Tp, float min_cos, float *__restrict__ x1out,
                              float *__restrict__ x2out, uint8_t *__restrict__ valid) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const float *T1w = Tp, *T2w = Tp + 12, *T21 = Tp + 24, *T2i = Tp + 36;
    const V3 xn1 = normalized(kb8_unproject(kb1, uv1[2 * i], uv1[2 * i + 1]));   // Mapping.cc:297-298
    const V3 xn2 = normalized(kb8_unproject(kb2, uv2[2 * i], uv2[2 * i + 1]));
    V3 p3D1, p3D2;
    tri_seed<METHOD, LOC>(xn1, xn2, T21, p3D1, p3D2);
    const V3 X1 = xform(T2i, p3D1), X2 = xform(T2i, p3D2);                    // T2w.inverse() * p
    // isValidParallax (Mapping.cc:351-366)
    const V3 c1 = xform(T1w, X1), c2 = xform(T2w, X2);
    const float cosp = cos_world_rays(T1w, T2w, xn1, xn2);
    valid[i] = (c1.z >= 0.0f && c2.z >= 0.0f && cosp <= min_cos && finite3(X1) && finite3(X2)) ? 1 : 0;
    x1out[3 * i] = X1.x; x1out[3 * i + 1] = X1.y; x1out[3 * i + 2] = X1.z;
    x2out[3 * i] = X2.x; x2out[3 * i + 1] = X2.y; x2out[3 * i + 2] = X2.z;
}

// squaredReprojectionError(x, KannalaBrandt8::project(pc)) (Geometry.cc:232-237)
__device__ __forceinline__ float sq_reprojection(const float *k, float u, float v, V3 pc) {
    const float p[3] = {pc.x, pc.y, pc.z};
    float uv[2];
    kb8_project(k, p, uv);
    const float ex = u - uv[0], ey = v - uv[1];
    return ex * ex + ey * ey;
}
// Eigen's float isZero(): every |coefficient| <= 1e-5
__device__ __forceinline__ bool is_zero3(V3 a) { return fabsf(a.x) <= 1e-5f && fabsf(a.y) <= 1e-5f && fabsf(a.z) <= 1e-5f; }

// MonocularMapInitializer::reconstructPoints, the loop body (MonocularMapInitializer.cc:303-367) for
// matched pixel pairs.  status: 0 kept, else the reference's first failing test (deftri.h)
template <int METHOD, int LOC>
__global__ void k_reconstruct_points(int n, const float *__restrict__ uv1, const float *__restrict__ uv2,
                                     const float *__restrict__ kb1, const float *__restrict__ kb2,
                                     const float *__restrict__ Tp, float depth_limit, int checks,
                                     float *__restrict__ x1out, float *__restrict__ x2out,
                                     uint8_t *__restrict__ status, float *__restrict__ cos_out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const float *T1w = Tp, *T2w = Tp + 12, *T21 = Tp + 24, *T2i = Tp + 36;
    const float u1 = uv1[2 * i], v1 = uv1[2 * i + 1], u2 = uv2[2 * i], v2 = uv2[2 * i + 1];
    const V3 r1 = normalized(kb8_unproject(kb1, u1, v1)), r2 = normalized(kb8_unproject(kb2, u2, v2));   // :308-309
    V3 p3D1, p3D2;
    tri_seed<METHOD, LOC>(r1, r2, T21, p3D1, p3D2);
    const V3 X1 = xform(T2i, p3D1), X2 = xform(T2i, p3D2);
    const V3 c1 = xform(T1w, X1), c2 = xform(T2w, X2);                          // :321-322
    const float cosp = cos_world_rays(T1w, T2w, r1, r2);                       // :324-326
    int st = 0;
    if (!finite3(X1) || !finite3(X2) || is_zero3(X1) || is_zero3(X2)) st = 1;                   // :315
    else if (c1.z < 0.0f || c1.z > depth_limit) st = 2;                                         // :329
    else if (checks && (double)sq_reprojection(kb1, u1, v1, c1) > 5.991) st = 3;                // :339
    else if (c2.z < 0.0f || c2.z > depth_limit) st = 4;                                         // :346
    else if (checks && (double)sq_reprojection(kb2, u2, v2, c2) > 5.991) st = 5;                // :355
    status[i] = (uint8_t)st;
    cos_out[i] = cosp;
    x1out[3 * i] = X1.x; x1out[3 * i + 1] = X1.y; x1out[3 * i + 2] = X1.z;
    x2out[3 * i] = X2.x; x2out[3 * i + 1] = X2.y; x2out[3 * i + 2] = X2.z;
}

// The initial estimatedDepthScale_ of the two keyframes (Mapping.cc:183-254) over the correspondences
// reconstructPoints kept.  Per correspondence: d = getDepthMeasure(x, y) of both images (the sampler of
// k_depth_sample); dropped (keep 0) where d <= 0 in either image or a pixel is outside (0.1, 1500),
// the reference's literals (:194-200).  pix_status: the sampler's status of pixel 1 | pixel 2 << 4 (the
// host fails the call on a non-zero one).  A kept correspondence whose parallax angle IN DEGREES is
// above min_cos — the reference compares degrees with Triangulation.minCos (:220); reproduced as it
// stands — adds getDepthMeasure(x, y, false) / z_c (double / float promoted to double, :227-228) to its
// keyframe's sum.  part [3 * gridDim.x]: per workgroup the two sums and the count, fp64, a butterfly per
// wave and then the four waves (k_trial_eval's idiom, no atomics); the host adds them in workgroup order.
__global__ void __launch_bounds__(256)
k_init_depth_scales(int n, const float *__restrict__ uv1, const float *__restrict__ uv2, const float *__restrict__ x3d1,
                    const float *__restrict__ x3d2, const float *__restrict__ kb1, const float *__restrict__ kb2,
                    const float *__restrict__ Tp, float min_cos, const float *__restrict__ img1, int rows1, int cols1,
                    double scale1, const float *__restrict__ img2, int rows2, int cols2, double scale2,
                    uint8_t *__restrict__ keep, uint8_t *__restrict__ pix_status, double *__restrict__ part) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    double acc[3] = {0.0, 0.0, 0.0};
    if (i < n) {
        const float *T1w = Tp, *T2w = Tp + 12;
        const float u1 = uv1[2 * i], v1 = uv1[2 * i + 1], u2 = uv2[2 * i], v2 = uv2[2 * i + 1];
        unsigned char s1, s2;
        const double d1 = depth_measure_px(img1, rows1, cols1, scale1, u1, v1, 1, &s1);      // :191-192
        const double d2 = depth_measure_px(img2, rows2, cols2, scale2, u2, v2, 1, &s2);
        pix_status[i] = (uint8_t)(s1 | (s2 << 4));
        bool k = !s1 && !s2 && !(d1 <= 0.0 || d2 <= 0.0);
        k = k && !((double)u1 <= 0.1 || u1 >= 1500.0f || (double)v1 <= 0.1 || v1 >= 1500.0f);
        k = k && !((double)u2 <= 0.1 || u2 >= 1500.0f || (double)v2 <= 0.1 || v2 >= 1500.0f);
        keep[i] = k ? 1 : 0;
        if (k) {
            const V3 r1 = normalized(kb8_unproject(kb1, u1, v1)), r2 = normalized(kb8_unproject(kb2, u2, v2));
            const float cosp = cos_world_rays(T1w, T2w, r1, r2);
            const float degrees = (float)((double)acosf(cosp) * (180.0 / 3.14159265358979323846));
            if (degrees > min_cos) {                                                       // degrees vs minCos
                unsigned char s;
                const double d1u = depth_measure_px(img1, rows1, cols1, scale1, u1, v1, 0, &s);
                const double d2u = depth_measure_px(img2, rows2, cols2, scale2, u2, v2, 0, &s);
                const V3 c1 = xform(T1w, v3(x3d1[3 * i], x3d1[3 * i + 1], x3d1[3 * i + 2]));
                const V3 c2 = xform(T2w, v3(x3d2[3 * i], x3d2[3 * i + 1], x3d2[3 * i + 2]));
                acc[0] = d1u / (double)c1.z;
                acc[1] = d2u / (double)c2.z;
                acc[2] = 1.0;
            }
        }
    }
    __shared__ double red[3][4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        double a = acc[q];
        for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
        if (lane == 0) red[q][w] = a;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double *r = red[threadIdx.x];
        part[3 * (size_t)blockIdx.x + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
    }
}
#pragma clang fp contract(on)

}  // namespace dev

namespace {
template <int METHOD>
bool triangulate_loc(int loc, int n, const float *uv1, const float *uv2, const float *kb1, const float *kb2, const float *Tp,
                     float min_cos, float *x1, float *x2, uint8_t *valid, hipStream_t st) {
    const dim3 g((n + 255) / 256), b(256);
#define TRI(L) hipLaunchKernelGGL((dev::k_triangulate<METHOD, L>), g, b, 0, st, n, uv1, uv2, kb1, kb2, Tp, min_cos, x1, x2, valid)
    switch (loc) {
        case DEFTRI_LOC_INRAYS: TRI(DEFTRI_LOC_INRAYS); return true;
        case DEFTRI_LOC_TWOPOINTS: TRI(DEFTRI_LOC_TWOPOINTS); return true;
        case DEFTRI_LOC_FARPOINTS: TRI(DEFTRI_LOC_FARPOINTS); return true;
    }
#undef TRI
    return false;
}
template <int METHOD>
bool reconstruct_loc(int loc, int n, const float *uv1, const float *uv2, const float *kb1, const float *kb2, const float *Tp,
                     float depth_limit, int checks, float *x1, float *x2, uint8_t *status, float *cosp, hipStream_t st) {
    const dim3 g((n + 255) / 256), b(256);
#define REC(L) hipLaunchKernelGGL((dev::k_reconstruct_points<METHOD, L>), g, b, 0, st, n, uv1, uv2, kb1, kb2, Tp, depth_limit, \
                                  checks, x1, x2, status, cosp)
    switch (loc) {
        case DEFTRI_LOC_INRAYS: REC(DEFTRI_LOC_INRAYS); return true;
        case DEFTRI_LOC_TWOPOINTS: REC(DEFTRI_LOC_TWOPOINTS); return true;
        case DEFTRI_LOC_FARPOINTS: REC(DEFTRI_LOC_FARPOINTS); return true;
    }
#undef REC
    return false;
}

// k_triangulate of (DEFTRI_TRI_*, DEFTRI_LOC_*).  false: the reference defines no such variant (nothing
// launched)
bool launch_triangulate(int method, int loc, int n, const float *uv1, const float *uv2, const float *kb1, const float *kb2,
                        const float *Tp, float min_cos, float *x1, float *x2, uint8_t *valid, hipStream_t st) {
    if (n <= 0) return true;
    // triangulateClassic has no FarPoints branch: its else is the in-rays seed (Geometry.cc:89-96)
    if (method == DEFTRI_TRI_CLASSIC)
        return triangulate_loc<DEFTRI_TRI_CLASSIC>(loc == DEFTRI_LOC_FARPOINTS ? DEFTRI_LOC_INRAYS : loc, n, uv1, uv2, kb1, kb2,
                                                   Tp, min_cos, x1, x2, valid, st);
    if (method == DEFTRI_TRI_NRSLAM)
        return triangulate_loc<DEFTRI_TRI_NRSLAM>(loc, n, uv1, uv2, kb1, kb2, Tp, min_cos, x1, x2, valid, st);
    return false;
}

// k_reconstruct_points likewise
bool launch_reconstruct_points(int method, int loc, int n, const float *uv1, const float *uv2, const float *kb1,
                               const float *kb2, const float *Tp, float depth_limit, int checks, float *x1, float *x2,
                               uint8_t *status, float *cosp, hipStream_t st) {
    if (n <= 0) return true;
    if (method == DEFTRI_TRI_CLASSIC)
        return reconstruct_loc<DEFTRI_TRI_CLASSIC>(loc == DEFTRI_LOC_FARPOINTS ? DEFTRI_LOC_INRAYS : loc, n, uv1, uv2, kb1, kb2,
                                                   Tp, depth_limit, checks, x1, x2, status, cosp, st);
    if (method == DEFTRI_TRI_NRSLAM)
        return reconstruct_loc<DEFTRI_TRI_NRSLAM>(loc, n, uv1, uv2, kb1, kb2, Tp, depth_limit, checks, x1, x2, status, cosp, st);
    if (method == DEFTRI_TRI_DEPTH)
        return reconstruct_loc<DEFTRI_TRI_DEPTH>(loc, n, uv1, uv2, kb1, kb2, Tp, depth_limit, checks, x1, x2, status, cosp, st);
    return false;
}

// T1w, T2w, T21 = T2w * T1w.inverse(), T2w.inverse() (3x4 each), as Sophus forms them
void triangulation_poses(const float *T1w, const float *T2w, float Tp[48]) {
    float T1i[12];
    std::memcpy(Tp, T1w, 12 * sizeof(float));
    std::memcpy(Tp + 12, T2w, 12 * sizeof(float));
    pose34_inverse(T1w, T1i);
    pose34_product(T2w, T1i, Tp + 24);
    pose34_inverse(T2w, Tp + 36);
}

// "" when the reference defines the variant, else why it does not
const char *undefined_seed(int32_t method, int32_t location, bool simulated) {
    if (method != DEFTRI_TRI_CLASSIC && method != DEFTRI_TRI_NRSLAM && method != DEFTRI_TRI_ORBSLAM && method != DEFTRI_TRI_DEPTH)
        return "unknown triangulation method";
    if (location != DEFTRI_LOC_INRAYS && location != DEFTRI_LOC_TWOPOINTS && location != DEFTRI_LOC_FARPOINTS)
        return "unknown seed location";
    if (method == DEFTRI_TRI_ORBSLAM)
        return "Triangulation.method ORBSLAM is undefined in the reference: triangulateORBSLAM (Geometry.cc:155-186) never "
               "writes x3D_1 / x3D_2";
    if (method == DEFTRI_TRI_DEPTH && simulated)
        return "Triangulation.method DepthMeasurement is undefined in the simulated entry: its inputs are "
               "CameraModel::unproject(x, d), an unset vector (CameraModel.h:128-135); it is defined in "
               "deftri_reconstruct_points (Geometry.cc:189-214)";
    return "";
}

// the inputs every triangulation kernel reads: the pixel pairs, both calibrations, the four poses
struct TriInputs {
    float *uv1, *uv2, *k1, *k2, *T;
    TriInputs(DevArena &A, size_t N) {
        A.add(&uv1, 2 * N); A.add(&uv2, 2 * N); A.add(&k1, 8); A.add(&k2, 8); A.add(&T, 48);
    }
    // after A.commit(); Tp stays the caller's until the stream is synchronized
    void upload(size_t N, const float *h_uv1, const float *h_uv2, const float *kb8_1, const float *kb8_2, const float *Tp,
                hipStream_t st) const {
        hipMemcpyAsync(uv1, h_uv1, 8 * N, hipMemcpyHostToDevice, st);
        hipMemcpyAsync(uv2, h_uv2, 8 * N, hipMemcpyHostToDevice, st);
        hipMemcpyAsync(k1, kb8_1, 32, hipMemcpyHostToDevice, st);
        hipMemcpyAsync(k2, kb8_2, 32, hipMemcpyHostToDevice, st);
        hipMemcpyAsync(T, Tp, 48 * sizeof(float), hipMemcpyHostToDevice, st);
    }
};

int fail(std::string &err, int code, const std::string &what) {
    err = what;
    return code;
}
}  // namespace

int triangulate(int device, hipStream_t st, int32_t n, int32_t method, int32_t location, const float *uv1, const float *uv2,
                const float *kb8_1, const float *kb8_2, const float *T1w, const float *T2w, float min_cos, float *x3d_1,
                float *x3d_2, uint8_t *valid, std::string &err) {
    const char *why = undefined_seed(method, location, true);
    if (*why) return fail(err, DEFTRI_E_ARG, why);
    if (device < 0) return fail(err, DEFTRI_E_NODEVICE, "host-only context");
    if (n == 0) return 0;
    hipSetDevice(device);
    float Tp[48];
    triangulation_poses(T1w, T2w, Tp);
    const size_t N = (size_t)n;
    DevArena A;
    TriInputs in(A, N);
    float *d_x1, *d_x2;
    uint8_t *d_v;
    A.add(&d_x1, 3 * N); A.add(&d_x2, 3 * N); A.add(&d_v, N);
    if (!A.commit()) return fail(err, DEFTRI_E_HIP, "triangulate: allocation failed");
    in.upload(N, uv1, uv2, kb8_1, kb8_2, Tp, st);
    if (!launch_triangulate(method, location, n, in.uv1, in.uv2, in.k1, in.k2, in.T, min_cos, d_x1, d_x2, d_v, st)) {
        hipStreamSynchronize(st);
        return fail(err, DEFTRI_E_ARG, "triangulate: no kernel for this (method, location)");
    }
    hipMemcpyAsync(x3d_1, d_x1, 12 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(x3d_2, d_x2, 12 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(valid, d_v, N, hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(err, DEFTRI_E_HIP, std::string("triangulate: ") + hipGetErrorString(e));
    return 0;
}

int reconstruct_points(int device, hipStream_t st, int32_t n, const float *uv1, const float *uv2, const float *kb8_1,
                       const float *kb8_2, const float *T1w, const float *T2w, const deftri_reconstruct_params &params,
                       float *x3d_1, float *x3d_2, uint8_t *status, float *cos_parallax, deftri_reconstruct_report *report,
                       std::string &err) {
    const char *why = undefined_seed(params.method, params.location, false);
    if (*why) return fail(err, DEFTRI_E_ARG, why);
    if (device < 0) return fail(err, DEFTRI_E_NODEVICE, "host-only context");
    std::memset(report, 0, sizeof(*report));
    if (n == 0) return 0;
    hipSetDevice(device);
    float Tp[48];
    triangulation_poses(T1w, T2w, Tp);
    const size_t N = (size_t)n;
    DevArena A;
    TriInputs in(A, N);
    float *d_x1, *d_x2, *d_c;
    uint8_t *d_s;
    A.add(&d_x1, 3 * N); A.add(&d_x2, 3 * N); A.add(&d_s, N); A.add(&d_c, N);
    if (!A.commit()) return fail(err, DEFTRI_E_HIP, "reconstruct_points: allocation failed");
    in.upload(N, uv1, uv2, kb8_1, kb8_2, Tp, st);
    if (!launch_reconstruct_points(params.method, params.location, n, in.uv1, in.uv2, in.k1, in.k2, in.T, params.depth_limit,
                                   params.checks ? 1 : 0, d_x1, d_x2, d_s, d_c, st)) {
        hipStreamSynchronize(st);
        return fail(err, DEFTRI_E_ARG, "reconstruct_points: no kernel for this (method, location)");
    }
    hipMemcpyAsync(x3d_1, d_x1, 12 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(x3d_2, d_x2, 12 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(status, d_s, N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(cos_parallax, d_c, 4 * N, hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(err, DEFTRI_E_HIP, std::string("reconstruct_points: ") + hipGetErrorString(e));
    // the acceptance (:370-394) from the copied-back status and cosines
    std::vector<float> par;
    int64_t *counters[6] = {nullptr, &report->n_nonfinite, &report->n_depth1, &report->n_err1, &report->n_depth2,
                            &report->n_err2};
    for (size_t i = 0; i < N; i++) {
        if (status[i] == 0) par.push_back(cos_parallax[i]);
        else if (status[i] <= 5) ++*counters[status[i]];
    }
    report->n_triangulated = 2 * (int64_t)par.size();
    if (par.empty()) return 0;
    const size_t idx = std::min<size_t>(50, par.size() - 1);
    std::nth_element(par.begin(), par.begin() + (std::ptrdiff_t)idx, par.end());      // sorted order's element idx
    const float cosp = par[idx];
    if (cosp < 0.0f || cosp > 1.0f) return 0;                 // "Parallax must be between 0 and 1": not accepted
    const float radians = acosf(cosp);
    const float degrees = (float)((double)radians * (180.0 / M_PI));
    report->parallax_deg = degrees;
    report->accepted = (report->n_triangulated >= 25 && degrees > params.min_parallax) ? 1 : 0;
    return 0;
}

int init_depth_scales(int device, hipStream_t st, DepthImages &images, int64_t kf_id_1, int64_t kf_id_2, int32_t n,
                      const float *uv1, const float *uv2, const float *x3d_1, const float *x3d_2, const float *kb8_1,
                      const float *kb8_2, const float *T1w, const float *T2w, float min_cos, uint8_t *keep, double *scale_1,
                      double *scale_2, int64_t *n_points, std::string &err) {
    if (device < 0) return fail(err, DEFTRI_E_NODEVICE, "host-only context");
    hipSetDevice(device);
    DepthImageDev im[2];
    const int64_t ids[2] = {kf_id_1, kf_id_2};
    for (int c = 0; c < 2; c++)
        if (!images.device_image(ids[c], &im[c].pixels, &im[c].rows, &im[c].cols, &im[c].scale))
            return fail(err, DEFTRI_E_ARG, "Depth image is not initialized: keyframe " + std::to_string(ids[c]));
    const size_t N = (size_t)n, nb = (N + 255) / 256;
    double sum[3] = {0, 0, 0};
    if (n > 0) {
        float Tp[48];
        triangulation_poses(T1w, T2w, Tp);
        DevArena A;
        TriInputs in(A, N);
        float *d_x1, *d_x2;
        uint8_t *d_keep, *d_st;
        double *d_part;
        A.add(&d_x1, 3 * N); A.add(&d_x2, 3 * N); A.add(&d_keep, N); A.add(&d_st, N); A.add(&d_part, 3 * nb);
        if (!A.commit()) return fail(err, DEFTRI_E_HIP, "init_depth_scales: allocation failed");
        std::vector<uint8_t> h_keep(N), h_st(N);
        std::vector<double> part(3 * nb);
        in.upload(N, uv1, uv2, kb8_1, kb8_2, Tp, st);
        hipMemcpyAsync(d_x1, x3d_1, 12 * N, hipMemcpyHostToDevice, st);
        hipMemcpyAsync(d_x2, x3d_2, 12 * N, hipMemcpyHostToDevice, st);
        // keep [n], pix_status [n], part [3 * ceil(n / 256)] = per workgroup sum 1, sum 2, count
        hipLaunchKernelGGL(dev::k_init_depth_scales, dim3((unsigned)nb), dim3(256), 0, st, n, in.uv1, in.uv2, d_x1, d_x2, in.k1,
                           in.k2, in.T, min_cos, im[0].pixels, im[0].rows, im[0].cols, im[0].scale, im[1].pixels, im[1].rows,
                           im[1].cols, im[1].scale, d_keep, d_st, d_part);
        hipMemcpyAsync(h_keep.data(), d_keep, N, hipMemcpyDeviceToHost, st);
        hipMemcpyAsync(h_st.data(), d_st, N, hipMemcpyDeviceToHost, st);
        hipMemcpyAsync(part.data(), d_part, 24 * nb, hipMemcpyDeviceToHost, st);
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(err, DEFTRI_E_HIP, std::string("init_depth_scales: ") + hipGetErrorString(e));
        for (size_t i = 0; i < N; i++) {
            if (!h_st[i]) continue;
            const int c = (h_st[i] & 15) ? 0 : 1;
            const float *px = (c ? uv2 : uv1) + 2 * i;
            char buf[200];
            std::snprintf(buf, sizeof(buf), "keyframe %lld correspondence %zu: pixel (%g, %g) %s", (long long)ids[c], i,
                          (double)px[0], (double)px[1],
                          ((c ? h_st[i] >> 4 : h_st[i] & 15) == 1) ? "is out of range of the depth image"
                                                                   : "reads outside the depth image");
            return fail(err, DEFTRI_E_ARG, buf);
        }
        for (size_t b = 0; b < nb; b++)                        // workgroup order
            for (int q = 0; q < 3; q++) sum[q] += part[3 * b + q];
        std::memcpy(keep, h_keep.data(), N);
    }
    *n_points = (int64_t)sum[2];
    *scale_1 = sum[0] / sum[2];                                // n_points == 0: 0 / 0 = NaN, as the reference (:250-251)
    *scale_2 = sum[1] / sum[2];
    return 0;
}

}  // namespace deftri

