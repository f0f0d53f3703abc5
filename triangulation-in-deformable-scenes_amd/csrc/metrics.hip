// metrics.hip — calculatePixelsStandDev (reference Modules/Utils/Geometry.cc:370-498) on the device.
//
// Per matched slot of a keyframe pair the reference projects the MapPoint with the homogeneous
// fp32 product T.matrix() * [p; 1] (:423-431), KB8-projects it in fp32 and accumulates
// |obs - uv| and its square in u and v for both cameras (:440-452).  One thread per match computes
// the two error vectors; each workgroup reduces its 256 matches in a fixed tree order into one
// partial of 8 doubles (sum |e| and sum e^2, u and v, camera 1 then 2); the host adds the partials
// of each pair in order and replays the reference's per-pair formulas (pixels_stand_dev).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "dev_arena.h"
#include "device_math.h"
#include "metrics.h"
#include "pose_host.h"

namespace deftri {
namespace dev {

// fp32, no contraction: Eigen's lazy 4x4 * 4x1 product, column by column (:426)
#pragma clang fp contract(off)
__device__ __forceinline__ void pix_err(const float *cam, const float *p, const float *obs, double e[2]) {
    // cam: R (row-major 3x3, from the fp32 unit quaternion), t (3), kb8 (8)
    float pc[3];
#pragma unroll
    for (int r = 0; r < 3; r++) pc[r] = ((cam[3 * r] * p[0] + cam[3 * r + 1] * p[1]) + cam[3 * r + 2] * p[2]) + cam[9 + r];
    float uv[2];
    kb8_project(cam + 12, pc, uv);
    e[0] = fabs((double)obs[0] - (double)uv[0]);
    e[1] = fabs((double)obs[1] - (double)uv[1]);
}

// matches [m0, m1) of one pair; block b of the launch covers matches blk_first[b] .. +256 within
// its pair (blocks never straddle pairs), camera slots c1/c2 of the pair
__global__ void __launch_bounds__(256) k_pix_partial(const int32_t *__restrict__ blk_first, const int32_t *__restrict__ blk_last,
                                                     const int32_t *__restrict__ blk_pair, const int32_t *__restrict__ pair_cams,
                                                     const float *__restrict__ cams, const float *__restrict__ pts,
                                                     const float *__restrict__ obs, double *__restrict__ part) {
    __shared__ double red[8][256];
    const int b = blockIdx.x;
    const int m = blk_first[b] + (int)threadIdx.x;
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (m < blk_last[b]) {
        const int pr = blk_pair[b];
        double e1[2], e2[2];
        pix_err(cams + 20 * pair_cams[2 * pr], pts + 6 * (int64_t)m, obs + 4 * (int64_t)m, e1);
        pix_err(cams + 20 * pair_cams[2 * pr + 1], pts + 6 * (int64_t)m + 3, obs + 4 * (int64_t)m + 2, e2);
        v[0] = e1[0]; v[1] = e1[1]; v[2] = e1[0] * e1[0]; v[3] = e1[1] * e1[1];
        v[4] = e2[0]; v[5] = e2[1]; v[6] = e2[0] * e2[0]; v[7] = e2[1] * e2[1];
    }
#pragma unroll
    for (int q = 0; q < 8; q++) red[q][threadIdx.x] = v[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int q = 0; q < 8; q++) red[q][threadIdx.x] += red[q][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 8) part[8 * (int64_t)b + threadIdx.x] = red[threadIdx.x][0];
}
#pragma clang fp contract(on)

}  // namespace dev

int pixels_stand_dev(int device, hipStream_t st, const deftri_map &map, deftri_pixels_error *out, std::string &err) {
    if (device < 0) { err = "host-only context"; return DEFTRI_E_NODEVICE; }
    hipSetDevice(device);
    const int K = map.n_keyframes;
    // per keyframe: R (fp32, Eigen toRotationMatrix of the fp32 unit quaternion), t, kb8
    std::vector<float> cams(20 * (size_t)std::max(K, 1));
    for (int k = 0; k < K; k++) {
        const deftri_keyframe &kf = map.keyframes[k];
        const float q[4] = {(float)kf.pose[0], (float)kf.pose[1], (float)kf.pose[2], (float)kf.pose[3]};
        float *c = &cams[20 * (size_t)k];
        quat_to_rotation(q, c);
        for (int i = 0; i < 3; i++) c[9 + i] = (float)kf.pose[4 + i];
        for (int i = 0; i < 8; i++) c[12 + i] = kf.kb8[i];
    }
    // matches of each pair in the reference's loop order (:386-416)
    std::vector<float> pts, obs;
    std::vector<int32_t> pair_cams, pair_first{0};
    for (int a = 0; a < K; a++)
        for (int b = a + 1; b < K; b++) {
            const deftri_keyframe &k1 = map.keyframes[b], &k2 = map.keyframes[a];
            pair_cams.push_back(b); pair_cams.push_back(a);
            const int n = std::min(k1.n_slots, k2.n_slots);
            for (int i = 0; i < n; i++) {
                if (k1.point_id[i] < 0 || k2.point_id[i] < 0) continue;
                const int o1 = k1.obs_index[i], o2 = k2.obs_index[i];
                if (o1 < 0 || o2 < 0) continue;
                if (o1 >= k1.n_obs || o2 >= k2.n_obs) { err = "observation index out of range"; return DEFTRI_E_ARG; }
                for (int q = 0; q < 3; q++) pts.push_back(k1.point_pos[3 * (int64_t)i + q]);
                for (int q = 0; q < 3; q++) pts.push_back(k2.point_pos[3 * (int64_t)i + q]);
                obs.push_back(k1.kp_uv[2 * (int64_t)o1]); obs.push_back(k1.kp_uv[2 * (int64_t)o1 + 1]);
                obs.push_back(k2.kp_uv[2 * (int64_t)o2]); obs.push_back(k2.kp_uv[2 * (int64_t)o2 + 1]);
            }
            pair_first.push_back((int32_t)(pts.size() / 6));
        }
    const int npair = (int)pair_cams.size() / 2;
    // 256-match blocks that never straddle pairs: first match, end, pair
    std::vector<int32_t> bf, bl, bp;
    for (int p = 0; p < npair; p++)
        for (int32_t s = pair_first[p]; s < pair_first[p + 1]; s += 256) {
            bf.push_back(s); bl.push_back(std::min(s + 256, pair_first[p + 1])); bp.push_back(p);
        }
    const int nblk = (int)bf.size();
    std::vector<double> part(8 * (size_t)std::max(nblk, 1), 0.0);
    if (nblk > 0) {
        DevArena A;
        double *d_part;
        float *d_cams, *d_pts, *d_obs;
        int32_t *d_bf, *d_bl, *d_bp, *d_pc;
        A.add(&d_part, part.size()); A.add(&d_cams, cams.size()); A.add(&d_pts, pts.size()); A.add(&d_obs, obs.size());
        A.add(&d_bf, bf.size()); A.add(&d_bl, bl.size()); A.add(&d_bp, bp.size()); A.add(&d_pc, pair_cams.size());
        if (!A.commit()) { err = "pixels_stand_dev: allocation failed"; return DEFTRI_E_HIP; }
        hipMemcpyAsync(d_cams, cams.data(), 4 * cams.size(), hipMemcpyHostToDevice, st);
        hipMemcpyAsync(d_pts, pts.data(), 4 * pts.size(), hipMemcpyHostToDevice, st);
        hipMemcpyAsync(d_obs, obs.data(), 4 * obs.size(), hipMemcpyHostToDevice, st);
        hipMemcpyAsync(d_bf, bf.data(), 4 * bf.size(), hipMemcpyHostToDevice, st);
        hipMemcpyAsync(d_bl, bl.data(), 4 * bl.size(), hipMemcpyHostToDevice, st);
        hipMemcpyAsync(d_bp, bp.data(), 4 * bp.size(), hipMemcpyHostToDevice, st);
        hipMemcpyAsync(d_pc, pair_cams.data(), 4 * pair_cams.size(), hipMemcpyHostToDevice, st);
        hipLaunchKernelGGL(dev::k_pix_partial, dim3(nblk), dim3(256), 0, st, d_bf, d_bl, d_bp, d_pc, d_cams, d_pts, d_obs, d_part);
        hipMemcpyAsync(part.data(), d_part, 8 * part.size(), hipMemcpyDeviceToHost, st);
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) { err = std::string("pixels_stand_dev: ") + hipGetErrorString(e); return DEFTRI_E_HIP; }
    }
    // the reference's per-pair formulas (:454-485); meanUV and nMatches carry over pairs
    double mUV1[2] = {0, 0}, mUV2[2] = {0, 0};
    double mC1 = 0, mC2 = 0, dC1 = 0, dC2 = 0;
    size_t nMatches = 0;
    for (int p = 0, blk = 0; p < npair; p++) {
        double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (; blk < nblk && bp[blk] == p; blk++)
            for (int q = 0; q < 8; q++) sum[q] += part[8 * (size_t)blk + q];
        nMatches += (size_t)(pair_first[p + 1] - pair_first[p]);
        const double nm = (double)nMatches;
        for (int q = 0; q < 2; q++) { mUV1[q] += sum[q]; mUV2[q] += sum[4 + q]; }
        for (int q = 0; q < 2; q++) { mUV1[q] /= nm; mUV2[q] /= nm; }
        mC1 = (mUV1[0] + mUV1[1]) / 2.0;
        mC2 = (mUV2[0] + mUV2[1]) / 2.0;
        dC1 = (std::sqrt(sum[2] / nm) + std::sqrt(sum[3] / nm)) / 2.0;
        dC2 = (std::sqrt(sum[6] / nm) + std::sqrt(sum[7] / nm)) / 2.0;
    }
    out->avgc1 = mC1; out->avgc2 = mC2; out->avg = (mC1 + mC2) / 2.0;
    out->desvc1 = dC1; out->desvc2 = dC2; out->desv = (dC1 + dC2) / 2.0;
    return 0;
}

}  // namespace deftri
