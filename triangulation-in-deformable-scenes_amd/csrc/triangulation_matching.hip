// triangulation_matching.hip — searchForTriangulation (Modules/Matching/DescriptorMatching.cc:255-328):
// for every keypoint of keyframe 1 that holds no map point, the keypoint of keyframe 2 without a map point
// at the smallest Hamming distance among those on its epipolar line; a keypoint of keyframe 2 goes to the
// row that reached it at the strictly smallest distance, earlier rows losing it (deftri.h restates the loop).
//
// A row's own search is order-free: bestDist only moves on a pair that passed every test, so the row ends
// at the minimum distance over the pairs that pass, the largest j among equals.  What couples the rows is
// vMatchedDistance: row i loses keypoint j to any earlier row that holds it at a distance <= its own, which
// needs the claims of all earlier rows, not one lowest-index table per keypoint.  So the device does the
// heavy, order-free part and the host the coupling:
//   k_tri_rays         one thread per keypoint of either frame: ray1 = (E unproject(uv1)).normalized(),
//                      ray2 = unproject(uv2).normalized()
//   k_tri_candidates   one 64-lane wave per searched row, its descriptor in registers, the lanes striding
//                      over j: the pairs with a free slot, dist <= min(50, th - 1) and the epipolar test
//                      passed.  Run twice: a count pass, then k_excl_scan over the rows' counts, then a fill
//                      pass that writes (j, dist) compacted per row in ascending j — the position inside a
//                      row comes from the wave's ballot and a prefix count, no atomics.
//   one download of the row offsets and the lists, then the reference's loop over the lists: O(candidates).
// A pair with dist >= th is left out: it could only raise a bestDist that is not accepted anyway.
// Frame 2's descriptors are not staged through LDS: a wave's step reads 64 consecutive descriptors (2 KB,
// coalesced), all of frame 2 is 64 KB at 2000 keypoints and stays in L2, and staging for the four waves of
// a workgroup would put a workgroup barrier into a loop whose waves leave at different times (occupied rows).
//
// Float arithmetic without contraction on both sides.  A host-only context and a device context differ in
// their libm (sinf, cosf, acosf): a decision differs only where err sits within those ulps of epipolar_th.
#include <hip/hip_runtime.h>

#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "dev_arena.h"
#include "dev_scan.h"
#include "device_math.h"
#include "matching_grid.h"
#include "triangulation_matching.h"

namespace deftri {

namespace dev {
#pragma clang fp contract(off)
struct TriCam { float E[9], k[8]; };
enum { TS_MATCHED = 0, TS_OCCUPIED = 1, TS_NONE = 2, TS_STOLEN = 3, TS_FLAG = 4 };

// :282: (E * unproject(uv).transpose()).normalized(); the unprojected ray is not normalized first
__host__ __device__ __forceinline__ V3 tri_ray1(const TriCam &C, float u, float v) {
    const V3 r = kb8_unproject(C.k, u, v);
    return eigen_normalized(v3(C.E[0] * r.x + C.E[1] * r.y + C.E[2] * r.z, C.E[3] * r.x + C.E[4] * r.y + C.E[5] * r.z,
                               C.E[6] * r.x + C.E[7] * r.y + C.E[8] * r.z));
}

// :300: unproject(uv).normalized(), with kf1's calibration (:267)
__host__ __device__ __forceinline__ V3 tri_ray2(const TriCam &C, float u, float v) { return eigen_normalized(kb8_unproject(C.k, u, v)); }

// :303-304: float err = fabs(M_PI/2 - acos(ray2.dot(ray1))); err < fEpipolarTh.  The dot product is a float,
// acos the float overload (using namespace std), the difference and fabs are double (M_PI/2 is a double), the
// result is rounded to the float err.  A NaN (a non-finite ray, or a dot product beyond 1) compares false.
__host__ __device__ __forceinline__ bool tri_epipolar_pass(V3 r1, V3 r2, float epipolar_th) {
    const float d = r2.x * r1.x + r2.y * r1.y + r2.z * r1.z;
    const float err = (float)fabs(M_PI / 2 - (double)acosf(d));
    return err < epipolar_th;
}

__global__ void k_tri_rays(int n1, int n2, TriCam C, const float *__restrict__ uv1, const float *__restrict__ uv2,
                           float4 *__restrict__ ray1, float4 *__restrict__ ray2) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t < n1) {
        const V3 r = tri_ray1(C, uv1[2 * t], uv1[2 * t + 1]);
        ray1[t] = make_float4(r.x, r.y, r.z, 0.0f);
    } else if (t - n1 < n2) {
        const int j = t - n1;
        const V3 r = tri_ray2(C, uv2[2 * j], uv2[2 * j + 1]);
        ray2[j] = make_float4(r.x, r.y, r.z, 0.0f);
    }
}

// One wave per row of frame 1 (4 per workgroup).  FILL == false: count[i] = the row's passing pairs.
// FILL == true: the pairs at start[i] .., in ascending j; an entry at or beyond `capacity` is not written.
// Every wave runs the same trip count over j, so the ballot is taken by all 64 lanes.
template <bool FILL>
__global__ void __launch_bounds__(256)
k_tri_candidates(int n1, int n2, const uint8_t *__restrict__ has1, const uint8_t *__restrict__ has2, const uint4 *__restrict__ desc1,
                 const uint4 *__restrict__ desc2, const float4 *__restrict__ ray1, const float4 *__restrict__ ray2, int max_dist,
                 float epipolar_th, unsigned long long *__restrict__ count, const unsigned long long *__restrict__ start,
                 unsigned long long capacity, int *__restrict__ cand_j, uint8_t *__restrict__ cand_d) {
    const int lane = threadIdx.x & 63;
    const int i = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (i >= n1) return;
    if (has1[i]) {                                           // :277
        if (!FILL && lane == 0) count[i] = 0;
        return;
    }
    const uint4 a0 = desc1[2 * (size_t)i], a1 = desc1[2 * (size_t)i + 1];
    const float4 q = ray1[i];
    const V3 r1 = v3(q.x, q.y, q.z);
    unsigned long long run = FILL ? start[i] : 0ull;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < n2; base += 64) {
        const int j = base + lane;
        bool pass = false;
        int d = 0;
        if (j < n2 && !has2[j]) {                            // :288
            d = hamming256(a0, a1, desc2[2 * (size_t)j], desc2[2 * (size_t)j + 1]);
            if (d <= max_dist) {                             // :293 and the acceptance :310
                const float4 p = ray2[j];
                pass = tri_epipolar_pass(r1, v3(p.x, p.y, p.z), epipolar_th);
            }
        }
        const unsigned long long vote = __ballot(pass);
        if (FILL && pass) {
            const unsigned long long at = run + (unsigned long long)__popcll(vote & below);
            if (at < capacity) {
                cand_j[at] = j;
                cand_d[at] = (uint8_t)d;
            }
        }
        run += (unsigned long long)__popcll(vote);
    }
    if (!FILL && lane == 0) count[i] = run;
}

}  // namespace dev

using namespace dev;

namespace {
// what the loop keeps between rows (:269-274); vMatchedDistance and vnMatches21 sized by n2 (deftri.h)
struct LoopState {
    std::vector<int32_t> matched_dist, match21;
    bool flag = false;                                       // vbMatched2[2]
    int32_t flag_row = -1, n_matches = 0;
    explicit LoopState(int32_t n2) : matched_dist((size_t)n2, INT_MAX), match21((size_t)n2, -1) {}
};

// :310-324 for row i with its search's result
void accept_row(const TriangulationMatchArgs &a, LoopState &s, int32_t i, int best, int32_t best_idx) {
    if (!(best < a.th)) {
        a.status[i] = TS_NONE;
        return;
    }
    const int32_t robbed = s.match21[best_idx];
    if (robbed >= 0) {                                       // :314-317
        a.matches[robbed] = -1;
        a.status[robbed] = TS_STOLEN;
        s.n_matches--;
    }
    a.matches[i] = best_idx;
    a.status[i] = TS_MATCHED;
    if (a.best_dist) a.best_dist[i] = best;
    s.match21[best_idx] = i;
    if (best == 2 && !s.flag) {                              // vbMatched2[bestDist] = true, read back as [2]
        s.flag = true;
        s.flag_row = i;
    }
    s.matched_dist[best_idx] = best;
    s.n_matches++;
}

void fill_report(const TriangulationMatchArgs &a, const LoopState &s, long long n_listed, int round_trips, double ms_device,
                 double ms_loop, double ms_total) {
    *a.n_matches = s.n_matches;
    if (!a.report) return;
    deftri_triangulation_match_report r;
    std::memset(&r, 0, sizeof(r));
    r.n1 = a.n1;
    r.n2 = a.n2;
    r.n_matches = s.n_matches;
    for (int32_t i = 0; i < a.n1; i++) switch (a.status[i]) {
            case TS_OCCUPIED: r.n_occupied++; break;
            case TS_NONE: r.n_unmatched++; break;
            case TS_STOLEN: r.n_stolen++; break;
            case TS_FLAG: r.n_flag_skipped++; break;
            default: break;
        }
    r.flag_row = s.flag_row;
    r.n_listed = n_listed;
    r.round_trips = round_trips;
    r.ms_device = ms_device;
    r.ms_loop = ms_loop;
    r.ms_total = ms_total;
    *a.report = r;
}
}  // namespace

int search_for_triangulation(int device, hipStream_t st, const TriangulationMatchArgs &a, std::string &err) {
    const auto t0 = std::chrono::steady_clock::now();
    if (a.th > 255) {
        err = "search_for_triangulation: th > 255: a row without a candidate keeps bestDist = 255 < th and the reference uses an "
              "uninitialised bestIdx (DescriptorMatching.cc:286, :310)";
        return DEFTRI_E_ARG;
    }
    const int32_t n1 = a.n1, n2 = a.n2;
    for (int32_t i = 0; i < n1; i++) {
        a.matches[i] = -1;                                   // :257
        a.status[i] = a.has_point1[i] ? TS_OCCUPIED : TS_NONE;
        if (a.best_dist) a.best_dist[i] = 255;
    }
    LoopState s(n2);
    if (n1 == 0 || n2 == 0) {
        fill_report(a, s, 0, 0, 0.0, 0.0, ms_since(t0));
        return 0;
    }
    TriCam C;
    std::memcpy(C.E, a.E, sizeof(C.E));
    std::memcpy(C.k, a.kb8, sizeof(C.k));
    const bool quirk = a.flag_quirk != 0;

    if (device < 0) {
        // the loop as it stands; ray2 of a keypoint is the same for every row and is computed once
        std::vector<V3> ray2((size_t)n2);
        for (int32_t j = 0; j < n2; j++)
            if (!a.has_point2[j]) ray2[j] = tri_ray2(C, a.uv2[2 * j], a.uv2[2 * j + 1]);
        for (int32_t i = 0; i < n1; i++) {
            if (a.has_point1[i]) continue;                                          // :277
            if (quirk && s.flag) {                                                  // :288: every j is passed over
                a.status[i] = TS_FLAG;
                continue;
            }
            const V3 ray1 = tri_ray1(C, a.uv1[2 * i], a.uv1[2 * i + 1]);            // :282
            int best = 255;
            int32_t best_idx = -1;
            for (int32_t j = 0; j < n2; j++) {
                if (a.has_point2[j]) continue;                                      // :288
                const int dist = hamming(a.desc1 + 32 * (size_t)i, a.desc2 + 32 * (size_t)j);
                if (dist > 50 || dist > best) continue;                             // :293
                if (s.matched_dist[j] <= dist) continue;                            // :296
                if (tri_epipolar_pass(ray1, ray2[j], a.epipolar_th)) {              // :303-307
                    best = dist;
                    best_idx = j;
                }
            }
            accept_row(a, s, i, best, best_idx);
        }
        const double total = ms_since(t0);
        fill_report(a, s, 0, 0, 0.0, total, total);
        return 0;
    }

    hipSetDevice(device);
    const size_t N1 = (size_t)n1, N2 = (size_t)n2;
    const int max_dist = a.th <= 0 ? -1 : std::min(50, (int)a.th - 1);
    // the first fill pass has room for 64 pairs a row and a little more; a call with more takes a second
    // pass into a buffer of the exact size
    const unsigned long long worst = (unsigned long long)N1 * N2;
    unsigned long long capacity = std::min(worst, 64ull * N1 + 4096ull);
    DevArena A;
    float *d_uv1, *d_uv2;
    uint4 *d_desc1, *d_desc2;
    uint8_t *d_has1, *d_has2, *d_cand_d;
    float4 *d_ray1, *d_ray2;
    unsigned long long *d_count, *d_start;
    int *d_cand_j;
    A.in(&d_uv1, a.uv1, 2 * N1); A.in(&d_uv2, a.uv2, 2 * N2); A.in(&d_desc1, a.desc1, 2 * N1); A.in(&d_desc2, a.desc2, 2 * N2);
    A.in(&d_has1, a.has_point1, N1); A.in(&d_has2, a.has_point2, N2); A.add(&d_ray1, N1); A.add(&d_ray2, N2);
    A.add(&d_count, N1); A.add(&d_start, N1 + 1); A.add(&d_cand_j, (size_t)capacity); A.add(&d_cand_d, (size_t)capacity);
    if (!A.commit(st)) {
        err = "search_for_triangulation: allocation failed";
        return DEFTRI_E_HIP;
    }
    const unsigned n_ray_blocks = (unsigned)((N1 + N2 + 255) / 256), n_row_blocks = (unsigned)((N1 + 3) / 4);
    hipLaunchKernelGGL(dev::k_tri_rays, dim3(n_ray_blocks), dim3(256), 0, st, n1, n2, C, d_uv1, d_uv2, d_ray1, d_ray2);
    hipLaunchKernelGGL(dev::k_tri_candidates<false>, dim3(n_row_blocks), dim3(256), 0, st, n1, n2, d_has1, d_has2, d_desc1, d_desc2,
                       d_ray1, d_ray2, max_dist, a.epipolar_th, d_count, d_start, capacity, d_cand_j, d_cand_d);
    launch_excl_scan<unsigned long long, 256>(n1, d_count, d_start, nullptr, st);
    hipLaunchKernelGGL(dev::k_tri_candidates<true>, dim3(n_row_blocks), dim3(256), 0, st, n1, n2, d_has1, d_has2, d_desc1, d_desc2,
                       d_ray1, d_ray2, max_dist, a.epipolar_th, d_count, d_start, capacity, d_cand_j, d_cand_d);
    std::vector<unsigned long long> start(N1 + 1);
    std::vector<int32_t> cand_j((size_t)capacity);
    std::vector<uint8_t> cand_d((size_t)capacity);
    hipMemcpyAsync(start.data(), d_start, 8 * (N1 + 1), hipMemcpyDeviceToHost, st);
    if (capacity) {
        hipMemcpyAsync(cand_j.data(), d_cand_j, 4 * (size_t)capacity, hipMemcpyDeviceToHost, st);
        hipMemcpyAsync(cand_d.data(), d_cand_d, (size_t)capacity, hipMemcpyDeviceToHost, st);
    }
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(err, "search_for_triangulation", e);
    int round_trips = 1;
    const unsigned long long total = start[N1];
    if (total > worst) {
        err = "search_for_triangulation: the candidate count exceeds n1 * n2";
        return DEFTRI_E_INTERNAL;
    }
    if (total > capacity) {
        DevArena B;
        int *d_j2;
        uint8_t *d_d2;
        B.add(&d_j2, (size_t)total); B.add(&d_d2, (size_t)total);
        if (!B.commit()) {
            err = "search_for_triangulation: allocation failed";
            return DEFTRI_E_HIP;
        }
        capacity = total;
        hipLaunchKernelGGL(dev::k_tri_candidates<true>, dim3(n_row_blocks), dim3(256), 0, st, n1, n2, d_has1, d_has2, d_desc1,
                           d_desc2, d_ray1, d_ray2, max_dist, a.epipolar_th, d_count, d_start, capacity, d_j2, d_d2);
        cand_j.resize((size_t)total);
        cand_d.resize((size_t)total);
        hipMemcpyAsync(cand_j.data(), d_j2, 4 * (size_t)total, hipMemcpyDeviceToHost, st);
        hipMemcpyAsync(cand_d.data(), d_d2, (size_t)total, hipMemcpyDeviceToHost, st);
        e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(err, "search_for_triangulation", e);
        round_trips++;
    }
    const double ms_device = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    // the loop over the lists: every listed pair has a free slot, dist <= min(50, th - 1) and passed the
    // epipolar test, so what is left of :287-308 are the two tests against the state
    for (int32_t i = 0; i < n1; i++) {
        if (a.has_point1[i]) continue;
        if (quirk && s.flag) {
            a.status[i] = TS_FLAG;
            continue;
        }
        int best = 255;
        int32_t best_idx = -1;
        for (unsigned long long k = start[i]; k < start[i + 1]; k++) {
            const int32_t j = cand_j[k];
            const int dist = cand_d[k];
            if (j < 0 || j >= n2) {
                err = "search_for_triangulation: a candidate list names no keypoint";
                return DEFTRI_E_INTERNAL;
            }
            if (dist > best) continue;
            if (s.matched_dist[j] <= dist) continue;
            best = dist;
            best_idx = j;
        }
        accept_row(a, s, i, best, best_idx);
    }
    fill_report(a, s, (long long)total, round_trips, ms_device, ms_since(t1), ms_since(t0));
    return 0;
}

}  // namespace deftri
