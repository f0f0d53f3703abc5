// projection_matching.hip — map points into a frame's keypoint slots by projection, and what the
// projection matcher reads of a map point.
//
// guidedMatching (reference Modules/Matching/DescriptorMatching.cc:101-162) and searchWithProjection
// (:164-253) project map points through the frame's pose and Kannala-Brandt model, take the frame's
// keypoints in a window of its feature grid (Frame::getFeaturesInArea, Frame.cc:288-323), skip the ones
// whose slot already holds a map point (:138-140, :230-232), keep the two smallest Hamming distances of
// the rest and claim the best one's slot when bestDist <= th && (float)bestDist < float(second) * 0.9.
// The skip makes point i depend on the claims of every accepted point before it.
//   k_prepare_points     one thread per point: view cosine, distance, predicted octave, projection, radius
//   k_match_round        one 64-lane wave per point, against the claims of the previous round
// The search of fuse (:330-428, deftri_fuse_search) is the same window search with every slot free and no
// claims, so one round of k_match_round is its result; its prepare step is prepare_fuse.
// Claims are resolved in rounds (deftri.h has the argument): claim[j] holds the lowest index of a point
// that claimed keypoint j in the previous round (-1: occupied before the call, INT_MAX: free); point i
// skips j iff claim[j] < i; accepted points write their index into the next round's table with
// atomicMin; the rounds end when no point's accepted keypoint changed.  After round r points 0 .. r - 1
// hold the sequential loop's results, so the fixed point is that loop's result.
//
// Map::updateOrientationAndDescriptor (Map.cc:270-321) for a batch of map points:
//   k_map_point_descriptors   one wave per map point; per observation a 257-bin histogram of its Hamming
//                             distances to all observations, the median read off the running count
//
// Float arithmetic without contraction on both sides; the host loops below are the sequential
// restatements a host-only context runs and the kernels are tested against.  A host-only context and a
// device context differ in their libm (atan2f, sinf, cosf, logf): by ulps in uv, and in a decision only
// where the input sits within those ulps of a threshold.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>

#include "dev_arena.h"
#include "device_math.h"
#include "matching_grid.h"
#include "pose_host.h"
#include "projection_matching.h"

namespace deftri {

namespace dev {
#pragma clang fp contract(off)
// the frame: Tcw row-major 3x4, the camera centre Tcw.inverse().translation(), KannalaBrandt8
struct ProjCam { float T[12], c[3], k[8]; };
// what the matchers' window search needs of a point
struct PointPrep {
    float x, y, radius, view_cos;
    int octave, status;          // status 0: search the window; else final (deftri.h)
};
enum { ST_MATCHED = 0, ST_VIEW_COS = 1, ST_INV_DIST = 2, ST_NO_CANDIDATES = 3, ST_REJECTED = 4, ST_UNDEFINED = 5, ST_EMPTY_SLOT = 6 };

// KannalaBrandt8::project (KannalaBrandt8.cc:32-49), device_math.h's kb8_project for host and device
__host__ __device__ __forceinline__ void kb8_project_hd(const float *k, V3 p, float &u, float &v) {
    const float x2_plus_y2 = p.x * p.x + p.y * p.y;
    const float theta = atan2f(sqrtf(x2_plus_y2), p.z);
    const float psi = atan2f(p.y, p.x);
    const float theta2 = theta * theta;
    const float theta3 = theta * theta2;
    const float theta5 = theta3 * theta2;
    const float theta7 = theta5 * theta2;
    const float theta9 = theta7 * theta2;
    const float r = theta + k[4] * theta3 + k[5] * theta5 + k[6] * theta7 + k[7] * theta9;
    u = k[0] * r * cosf(psi) + k[2];
    v = k[1] * r * sinf(psi) + k[3];
}

// Tcw * X (Sophus: R X + t) and its projection
__host__ __device__ __forceinline__ void project_world(const ProjCam &C, V3 X, float &u, float &v) {
    const V3 pc = v3((C.T[0] * X.x + C.T[1] * X.y + C.T[2] * X.z) + C.T[3], (C.T[4] * X.x + C.T[5] * X.y + C.T[6] * X.z) + C.T[7],
                     (C.T[8] * X.x + C.T[9] * X.y + C.T[10] * X.z) + C.T[11]);
    kb8_project_hd(C.k, pc, u, v);
}

__host__ __device__ __forceinline__ bool finite2(float a, float b) { return fabsf(a) <= 3.402823466e38f && fabsf(b) <= 3.402823466e38f; }

// searchWithProjection :175-210 for one map point.  scale: vScaleFactor_ [n_scales]; log_scale1:
// log(getScaleFactor(1)) in float.  uv and view_cos are computed for every point.
__host__ __device__ __forceinline__ PointPrep prepare_projection(const ProjCam &C, V3 X, V3 normal, float min_dist, float max_dist,
                                                                 int n_scales, const float *scale, float log_scale1) {
    PointPrep p;
    p.radius = 0.0f;
    p.octave = -1;
    project_world(C, X, p.x, p.y);                                                  // :203-204
    const V3 ray = sub(X, v3(C.c[0], C.c[1], C.c[2]));                              // :177
    p.view_cos = dot(eigen_normalized(ray), normal);                                // :178
    if (p.view_cos < 0.5f) { p.status = ST_VIEW_COS; return p; }                    // :180
    const float dist = nrm(ray);                                                    // :186
    if (dist < min_dist || dist > max_dist) { p.status = ST_INV_DIST; return p; }   // :190
    const float c = ceilf(logf(max_dist / dist) / log_scale1);                      // :196, the float overloads
    // :197-200: clamped to [0, nScales]; a NaN has no int value and is undefined like nScales itself
    int octave;
    if (c != c || c > (float)n_scales) octave = n_scales;
    else if (c < 0.0f) octave = 0;
    else octave = (int)c;
    p.octave = octave;
    if (octave >= n_scales) { p.status = ST_UNDEFINED; return p; }                  // vScaleFactor_[nScales]: past the end
    if (!finite2(p.x, p.y)) { p.status = ST_UNDEFINED; return p; }                  // posInGrid's int conversion
    const float radius = scale[octave];                                            // :206-210, the products in double
    p.radius = (float)((double)radius * ((double)p.view_cos > 0.998 ? 2.5 : 4.0));
    p.status = 0;
    return p;
}

// guidedMatching :116-127 for one reference slot that holds a map point
__host__ __device__ __forceinline__ PointPrep prepare_guided(const ProjCam &C, V3 X, int octave, int window15, const float *scale) {
    PointPrep p;
    p.view_cos = 0.0f;
    p.octave = octave;
    project_world(C, X, p.x, p.y);
    p.radius = (float)window15 * scale[octave];                                    // 15 * windowSizeFactor is an int
    p.status = finite2(p.x, p.y) ? 0 : ST_UNDEFINED;
    return p;
}

// fuse :362-369 for one considered map point: no depth test, radius = 2.5 * getScaleFactor(octave) in double
__host__ __device__ __forceinline__ PointPrep prepare_fuse(const ProjCam &C, V3 X, int octave, const float *scale) {
    PointPrep p;
    p.view_cos = 0.0f;
    p.octave = octave;
    project_world(C, X, p.x, p.y);
    p.radius = (float)(2.5 * (double)scale[octave]);
    p.status = finite2(p.x, p.y) ? 0 : ST_UNDEFINED;
    return p;
}

enum { MODE_PROJECTION = 0, MODE_GUIDED = 1, MODE_FUSE = 2 };

struct PrepOut {
    float *x, *y, *radius, *view_cos;
    int *octave, *match, *best, *second;
    uint8_t *status;
};

__global__ void k_prepare_points(int n, int mode, ProjCam C, const float *__restrict__ pos, const float *__restrict__ normal,
                                 const float *__restrict__ min_dist, const float *__restrict__ max_dist,
                                 const uint8_t *__restrict__ has_point, const int *__restrict__ octave1, int window15, int n_scales,
                                 const float *__restrict__ scale, float log_scale1, PrepOut o) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    PointPrep p;
    const V3 X = v3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
    if (mode != MODE_PROJECTION) {
        if (has_point[i]) p = mode == MODE_FUSE ? prepare_fuse(C, X, octave1[i], scale) : prepare_guided(C, X, octave1[i], window15, scale);
        else { p.x = p.y = p.radius = p.view_cos = 0.0f; p.octave = -1; p.status = ST_EMPTY_SLOT; }
    } else {
        p = prepare_projection(C, X, v3(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]), min_dist[i], max_dist[i], n_scales,
                               scale, log_scale1);
    }
    o.x[i] = p.x; o.y[i] = p.y; o.radius[i] = p.radius; o.view_cos[i] = p.view_cos;
    o.octave[i] = p.octave;
    o.status[i] = (uint8_t)p.status;
    o.match[i] = -1; o.best[i] = 255; o.second[i] = 255;
}

// One wave per point (4 per workgroup), as k_match_init (wave_window_best).  claim_prev: the previous
// round's table; a candidate with claim_prev[j] < i is skipped entirely (:138-140, :230-232) but counts as a
// candidate for the emptiness test (:220).  match [n] holds the previous round's result on entry.
__global__ void __launch_bounds__(256)
k_match_round(int n, const float *__restrict__ px, const float *__restrict__ py, const float *__restrict__ pradius,
              const int *__restrict__ poctave, const uint4 *__restrict__ desc, const float *__restrict__ uv2,
              const int *__restrict__ octave2, const uint4 *__restrict__ desc2, GridGeom G, const int *__restrict__ cell_start,
              const int *__restrict__ cell_keys, int th, const int *__restrict__ claim_prev, int *__restrict__ claim_next,
              int *__restrict__ match, int *__restrict__ best_out, int *__restrict__ second_out, uint8_t *__restrict__ status,
              int *__restrict__ changed) {
    const int lane = threadIdx.x & 63;
    const int i = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (i >= n) return;
    const int st0 = status[i];
    if (st0 != ST_MATCHED && st0 != ST_NO_CANDIDATES && st0 != ST_REJECTED) return;   // decided by k_prepare_points
    const WindowBest w = wave_window_best(G, cell_start, cell_keys, uv2, octave2, desc2, px[i], py[i], pradius[i], poctave[i],
                                          desc[2 * (size_t)i], desc[2 * (size_t)i + 1], lane,
                                          [=](int j) { return claim_prev[j] < i; });   // getMapPoint(j)
    if (lane == 0) {
        const bool ok = w.ncand > 0 && accept_match(w.best, w.second, th);
        const int m = ok ? w.idx : -1;
        status[i] = (uint8_t)(w.ncand == 0 ? ST_NO_CANDIDATES : ok ? ST_MATCHED : ST_REJECTED);
        best_out[i] = w.best;
        second_out[i] = w.second;
        if (m != match[i]) {
            match[i] = m;
            *changed = 1;
        }
        if (m >= 0) atomicMin(&claim_next[m], i);
    }
}

// the lanes of one wave see each other's LDS accesses in program order; this keeps the compiler from moving
// any across (the waves of a workgroup run different trip counts, so there is no workgroup barrier)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Map::updateOrientationAndDescriptor, one wave per map point (4 per workgroup).  The normal and the
// chosen observation's distance are evaluated by every lane alike, in observation order.  Per
// observation i the lanes stride over j, count its distances in the wave's 257 bins, and the element
// nth_element puts at nObs / 2 is the first bin at which the running count exceeds nObs / 2.
// status: 0 written, 1 no observation, 2 the chosen ordinal is no slot of its keyframe (nothing written).
__global__ void __launch_bounds__(256)
k_map_point_descriptors(int n, const float *__restrict__ pos, const int *__restrict__ obs_start, const int *__restrict__ obs_kf,
                        const int *__restrict__ obs_slot, const float *__restrict__ kf_centre, const int *__restrict__ kf_slot_start,
                        const uint4 *__restrict__ kf_desc, const int *__restrict__ kf_octave, int n_scales,
                        const float *__restrict__ scale, float *__restrict__ normal, float *__restrict__ max_dist,
                        float *__restrict__ min_dist, uint4 *__restrict__ desc, int *__restrict__ ref_obs,
                        uint8_t *__restrict__ status) {
    __shared__ int hist_all[4][320];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int p = (int)(blockIdx.x * 4 + w);
    if (p >= n) return;                                      // whole waves leave; no workgroup barrier below
    int *hist = hist_all[w];
    const int o0 = obs_start[p], nobs = obs_start[p + 1] - o0;
    if (nobs <= 0) {
        if (lane == 0) { status[p] = 1; ref_obs[p] = -1; }
        return;
    }
    const V3 X = v3(pos[3 * p], pos[3 * p + 1], pos[3 * p + 2]);
    V3 nsum = v3(0.0f, 0.0f, 0.0f);
    for (int i = 0; i < nobs; i++) {                         // Map.cc:286-287
        const int kf = obs_kf[o0 + i];
        const V3 ray = sub(X, v3(kf_centre[3 * kf], kf_centre[3 * kf + 1], kf_centre[3 * kf + 2]));
        nsum = add(nsum, eigen_normalized(ray));
    }
    const float cnt = (float)nobs;
    const V3 nrml = eigen_normalized(v3(nsum.x / cnt, nsum.y / cnt, nsum.z / cnt));   // :293
    const int mid = nobs / 2;
    float best_median = 255.0f;                              // :296
    int obs_idx = 0;
    for (int i = 0; i < nobs; i++) {
        for (int k = lane; k < 320; k += 64) hist[k] = 0;
        wave_lds_sync();
        const size_t di = (size_t)kf_slot_start[obs_kf[o0 + i]] + obs_slot[o0 + i];
        const uint4 a0 = kf_desc[2 * di], a1 = kf_desc[2 * di + 1];
        for (int j = lane; j < nobs; j += 64) {
            const size_t dj = (size_t)kf_slot_start[obs_kf[o0 + j]] + obs_slot[o0 + j];
            atomicAdd(&hist[hamming256(a0, a1, kf_desc[2 * dj], kf_desc[2 * dj + 1])], 1);
        }
        wave_lds_sync();
        // lane l owns bins 5 l .. 5 l + 4 (320 >= 257); the median is in the first lane whose inclusive
        // running count exceeds mid
        int h[5], own = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) { h[k] = hist[5 * lane + k]; own += h[k]; }
        int incl = own;
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        const unsigned long long over = __ballot(incl > mid);
        const int src = __ffsll((long long)over) - 1;        // over != 0: the last lane's count is nobs > mid
        int run = incl - own, med = 5 * lane;
#pragma unroll
        for (int k = 4; k >= 0; k--) {
            int below = run;
            for (int q = 0; q < k; q++) below += h[q];
            if (below <= mid && below + h[k] > mid) med = 5 * lane + k;
        }
        med = __shfl(med, src, 64);
        if ((float)med < best_median) {                      // :304-307
            best_median = (float)med;
            obs_idx = i;
        }
        wave_lds_sync();
    }
    const int kf = obs_kf[o0 + obs_idx];
    const int kf_slots = kf_slot_start[kf + 1] - kf_slot_start[kf];
    if (obs_idx >= kf_slots) {                               // :312 reads keypoint obsIdx, the ordinal
        if (lane == 0) { status[p] = 2; ref_obs[p] = obs_idx; }
        return;
    }
    const float dist = nrm(sub(X, v3(kf_centre[3 * kf], kf_centre[3 * kf + 1], kf_centre[3 * kf + 2])));   // :311
    const int ref_octave = kf_octave[kf_slot_start[kf] + obs_idx];
    const float mx = dist * scale[ref_octave];               // :314-315
    const float mn = mx / scale[n_scales - 1];
    if (lane == 0) {
        normal[3 * p] = nrml.x; normal[3 * p + 1] = nrml.y; normal[3 * p + 2] = nrml.z;
        max_dist[p] = mx;
        min_dist[p] = mn;
        const size_t d = (size_t)kf_slot_start[kf] + obs_slot[o0 + obs_idx];
        desc[2 * (size_t)p] = kf_desc[2 * d];
        desc[2 * (size_t)p + 1] = kf_desc[2 * d + 1];
        ref_obs[p] = obs_idx;
        status[p] = 0;
    }
}

}  // namespace dev

using namespace dev;

namespace {
// vScaleFactor_ (Frame.cc:65-70)
std::vector<float> scale_table(int n_scales, float factor) {
    std::vector<float> s((size_t)n_scales);
    s[0] = 1.0f;
    for (int i = 1; i < n_scales; i++) s[i] = s[i - 1] * factor;
    return s;
}

ProjCam camera_of(const float *Tcw, const float *kb8) {
    ProjCam C;
    float Ti[12];
    std::memcpy(C.T, Tcw, sizeof(C.T));
    std::memcpy(C.k, kb8, sizeof(C.k));
    pose34_inverse(Tcw, Ti);                                 // getPose().inverse().translation()
    C.c[0] = Ti[3]; C.c[1] = Ti[7]; C.c[2] = Ti[11];
    return C;
}

void fill_report(const ProjectionMatchArgs &a, int rounds, int round_trips, double ms_setup, double ms_rounds, double ms_total) {
    if (!a.report) return;
    deftri_projection_report r;
    std::memset(&r, 0, sizeof(r));
    r.n_points = a.n;
    for (int32_t i = 0; i < a.n; i++) switch (a.status[i]) {
            case ST_MATCHED: r.n_matches++; break;
            case ST_VIEW_COS: r.n_view_cos++; break;
            case ST_INV_DIST: r.n_inv_dist++; break;
            case ST_NO_CANDIDATES: r.n_no_candidates++; break;
            case ST_REJECTED: r.n_rejected++; break;
            case ST_UNDEFINED: r.n_undefined++; break;
            default: break;
        }
    r.rounds = rounds;
    r.round_trips = round_trips;
    r.ms_setup = ms_setup;
    r.ms_rounds = ms_rounds;
    r.ms_total = ms_total;
    *a.report = r;
}
}  // namespace

int projection_match(int device, hipStream_t st, const ProjectionMatchArgs &a, std::string &err) {
    const auto t0 = std::chrono::steady_clock::now();
    const char *name = a.fuse ? "fuse_search" : a.guided ? "guided_matching" : "search_with_projection";
    const deftri_feature_grid &grid = *a.grid;
    const std::string why = grid_error(grid);
    if (!why.empty()) {
        err = std::string(name) + ": " + why;
        return DEFTRI_E_ARG;
    }
    if (!a.guided && grid.n_scales < 2) {
        err = std::string(name) + ": FeatureExtractor.nScales < 2: the reference reads getScaleFactor(1) (DescriptorMatching.cc:196)";
        return DEFTRI_E_ARG;
    }
    if (a.guided && (a.window_size_factor < 0 || a.window_size_factor > (1 << 20))) {
        err = std::string(name) + ": windowSizeFactor outside [0, 2^20]";
        return DEFTRI_E_ARG;
    }
    if (!octaves_ok(name, "current keypoint", grid, a.n2, a.octave2, nullptr, err)) return DEFTRI_E_ARG;
    if (a.guided && !octaves_ok(name, a.fuse ? "map point" : "reference keypoint", grid, a.n, a.octave1, a.has_point, err))
        return DEFTRI_E_ARG;
    if (a.n == 0 || a.n2 == 0) {                              // nothing beyond the report
        if (a.report) {
            std::memset(a.report, 0, sizeof(*a.report));
            a.report->ms_total = ms_since(t0);
        }
        return 0;
    }
    const GridGeom G = geometry(grid);
    const ProjCam C = camera_of(a.Tcw, a.kb8);
    const std::vector<float> scale = scale_table(grid.n_scales, grid.scale_factor);
    const float log_scale1 = grid.n_scales > 1 ? logf(scale[1]) : 0.0f;
    const int window15 = 15 * a.window_size_factor;
    const int32_t n = a.n, n2 = a.n2;
    // a slot that holds anything but -1 on entry is occupied and keeps its value
    std::vector<int32_t> slot_in((size_t)n2, -1);
    if (!a.guided) std::memcpy(slot_in.data(), a.slot_point, sizeof(int32_t) * (size_t)n2);   // guidedMatching: clearMapPoints (:102)

    if (device < 0) {
        const auto cells = host_grid(G, n2, a.uv2);
        std::vector<int32_t> slot = slot_in;
        for (int32_t i = 0; i < n; i++) {
            const V3 X = v3(a.pos[3 * i], a.pos[3 * i + 1], a.pos[3 * i + 2]);
            PointPrep p;
            if (a.guided) {
                if (a.has_point[i])
                    p = a.fuse ? prepare_fuse(C, X, a.octave1[i], scale.data()) : prepare_guided(C, X, a.octave1[i], window15, scale.data());
                else { p.x = p.y = p.radius = p.view_cos = 0.0f; p.octave = -1; p.status = ST_EMPTY_SLOT; }
            } else {
                p = prepare_projection(C, X, v3(a.normal[3 * i], a.normal[3 * i + 1], a.normal[3 * i + 2]), a.min_dist[i],
                                       a.max_dist[i], grid.n_scales, scale.data(), log_scale1);
            }
            WindowBest w{255, 255, -1, 0};
            int status = p.status;
            int32_t m = -1;
            if (status == 0) {
                w = host_window_best(G, cells, a.uv2, a.octave2, a.desc2, p.x, p.y, p.radius, p.octave, a.desc + 32 * (size_t)i,
                                     [&](int32_t j) { return slot[j] != -1; });   // :230-232
                if (w.ncand == 0) status = ST_NO_CANDIDATES;                  // :220
                else if (accept_match(w.best, w.second, a.th)) {              // :246-249
                    if (!a.fuse) slot[w.idx] = i;                             // fuse: the slots are the caller's to edit
                    m = w.idx;
                    status = ST_MATCHED;
                } else status = ST_REJECTED;
            }
            a.match[i] = m;
            a.status[i] = (uint8_t)status;
            if (a.uv) { a.uv[2 * i] = p.x; a.uv[2 * i + 1] = p.y; }
            if (a.view_cos) a.view_cos[i] = p.view_cos;
            if (a.predicted_octave) a.predicted_octave[i] = p.octave;
            if (a.best) a.best[i] = w.best;
            if (a.second) a.second[i] = w.second;
        }
        if (a.slot_point) std::memcpy(a.slot_point, slot.data(), sizeof(int32_t) * (size_t)n2);
        const double total = ms_since(t0);
        fill_report(a, 1, 0, 0.0, total, total);
        return 0;
    }

    hipSetDevice(device);
    const size_t N = (size_t)n, N2 = (size_t)n2, ncell = (size_t)G.cols * G.rows;
    DevArena A;
    float *d_pos, *d_normal, *d_min, *d_max, *d_uv2, *d_scale, *d_x, *d_y, *d_radius, *d_cos;
    int *d_oct1, *d_oct2, *d_cell, *d_keys, *d_count, *d_cursor, *d_start, *d_octave, *d_match, *d_best, *d_second;
    int *d_base, *d_claim[2], *d_changed;
    uint8_t *d_has, *d_status;
    uint4 *d_desc, *d_desc2;
    std::vector<int32_t> base(N2);
    for (size_t j = 0; j < N2; j++) base[j] = slot_in[j] != -1 ? -1 : INT_MAX;
    A.in(&d_pos, a.pos, 3 * N);
    if (a.guided) {                                           // each mode uploads what its prepare step reads
        A.add(&d_normal, 3 * N); A.add(&d_min, N); A.add(&d_max, N); A.in(&d_has, a.has_point, N); A.in(&d_oct1, a.octave1, N);
    } else {
        A.in(&d_normal, a.normal, 3 * N); A.in(&d_min, a.min_dist, N); A.in(&d_max, a.max_dist, N); A.add(&d_has, N); A.add(&d_oct1, N);
    }
    A.in(&d_desc, a.desc, 2 * N); A.in(&d_scale, scale.data(), scale.size());
    A.in(&d_uv2, a.uv2, 2 * N2); A.in(&d_oct2, a.octave2, N2); A.in(&d_desc2, a.desc2, 2 * N2);
    A.add(&d_cell, N2); A.add(&d_keys, N2); A.add(&d_count, ncell); A.add(&d_cursor, ncell); A.add(&d_start, ncell + 1);
    A.add(&d_x, N); A.add(&d_y, N); A.add(&d_radius, N); A.add(&d_cos, N); A.add(&d_octave, N); A.add(&d_status, N);
    A.add(&d_match, N); A.add(&d_best, N); A.add(&d_second, N);
    A.in(&d_base, base.data(), N2); A.add(&d_claim[0], N2); A.add(&d_claim[1], N2); A.add(&d_changed, 1);
    if (!A.commit(st)) {
        err = std::string(name) + ": allocation failed";
        return DEFTRI_E_HIP;
    }
    hipMemcpyAsync(d_claim[0], d_base, 4 * N2, hipMemcpyDeviceToDevice, st);   // after d_base's upload
    launch_grid(G, n2, d_uv2, d_cell, d_count, d_start, d_cursor, d_keys, st);
    const PrepOut po{d_x, d_y, d_radius, d_cos, d_octave, d_match, d_best, d_second, d_status};
    hipLaunchKernelGGL(dev::k_prepare_points, dim3((n + 255) / 256), dim3(256), 0, st, n,
                       a.fuse ? (int)MODE_FUSE : a.guided ? (int)MODE_GUIDED : (int)MODE_PROJECTION, C, d_pos, d_normal, d_min, d_max,
                       d_has, d_oct1, window15, (int)grid.n_scales, d_scale, log_scale1, po);
    const double ms_setup = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    // the rounds: round r reads claim[(r - 1) & 1] and writes claim[r & 1]; one flag read each
    int rounds = 0, round_trips = 0, changed = 1;
    if (a.fuse) {
        // every slot is free and stays free: one round is the result, read back with the results
        hipMemsetAsync(d_changed, 0, sizeof(int), st);
        hipMemcpyAsync(d_claim[1], d_base, 4 * N2, hipMemcpyDeviceToDevice, st);
        hipLaunchKernelGGL(dev::k_match_round, dim3((n + 3) / 4), dim3(256), 0, st, n, d_x, d_y, d_radius, d_octave, d_desc, d_uv2,
                           d_oct2, d_desc2, G, d_start, d_keys, a.th, d_claim[0], d_claim[1], d_match, d_best, d_second, d_status,
                           d_changed);
        rounds = 1;
        changed = 0;
    }
    while (changed && rounds <= n) {
        int *prev = d_claim[rounds & 1], *next = d_claim[(rounds + 1) & 1];
        hipMemsetAsync(d_changed, 0, sizeof(int), st);
        hipMemcpyAsync(next, d_base, 4 * N2, hipMemcpyDeviceToDevice, st);
        hipLaunchKernelGGL(dev::k_match_round, dim3((n + 3) / 4), dim3(256), 0, st, n, d_x, d_y, d_radius, d_octave, d_desc, d_uv2,
                           d_oct2, d_desc2, G, d_start, d_keys, a.th, prev, next, d_match, d_best, d_second, d_status, d_changed);
        hipMemcpyAsync(&changed, d_changed, sizeof(int), hipMemcpyDeviceToHost, st);
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(err, name, e);
        rounds++;
        round_trips++;
    }
    if (changed) {
        err = std::string(name) + ": the claims did not settle in n + 1 rounds";
        return DEFTRI_E_INTERNAL;
    }
    const double ms_rounds = ms_since(t1);
    std::vector<int32_t> claim(N2), oct(N);
    std::vector<float> x(N), y(N);
    hipMemcpyAsync(claim.data(), d_claim[rounds & 1], 4 * N2, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(a.match, d_match, 4 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(a.status, d_status, N, hipMemcpyDeviceToHost, st);
    if (a.uv) {
        hipMemcpyAsync(x.data(), d_x, 4 * N, hipMemcpyDeviceToHost, st);
        hipMemcpyAsync(y.data(), d_y, 4 * N, hipMemcpyDeviceToHost, st);
    }
    if (a.view_cos) hipMemcpyAsync(a.view_cos, d_cos, 4 * N, hipMemcpyDeviceToHost, st);
    if (a.predicted_octave) hipMemcpyAsync(a.predicted_octave, d_octave, 4 * N, hipMemcpyDeviceToHost, st);
    if (a.best) hipMemcpyAsync(a.best, d_best, 4 * N, hipMemcpyDeviceToHost, st);
    if (a.second) hipMemcpyAsync(a.second, d_second, 4 * N, hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(err, name, e);
    round_trips++;
    if (a.uv)
        for (size_t i = 0; i < N; i++) { a.uv[2 * i] = x[i]; a.uv[2 * i + 1] = y[i]; }
    for (size_t j = 0; a.slot_point && j < N2; j++) a.slot_point[j] = slot_in[j] != -1 ? slot_in[j] : (claim[j] == INT_MAX ? -1 : claim[j]);
    fill_report(a, rounds, round_trips, ms_setup, ms_rounds, ms_since(t0));
    return 0;
}

int map_point_descriptors(int device, hipStream_t st, int32_t n, const float *pos, const int32_t *obs_start, const int32_t *obs_kf,
                          const int32_t *obs_slot, int32_t n_kf, const float *kf_Tcw, const int32_t *kf_slot_start,
                          const uint8_t *kf_desc, const int32_t *kf_octave, int32_t n_scales, float scale_factor, float *normal,
                          float *max_dist, float *min_dist, uint8_t *desc, int32_t *ref_obs, uint8_t *status, std::string &err) {
    const char *name = "map_point_descriptors";
    if (n_scales < 1) {
        err = std::string(name) + ": FeatureExtractor.nScales < 1";
        return DEFTRI_E_ARG;
    }
    if (n == 0) return 0;
    if (obs_start[0] != 0 || kf_slot_start[0] != 0) {
        err = std::string(name) + ": obs_start[0] and kf_slot_start[0] must be 0";
        return DEFTRI_E_ARG;
    }
    for (int32_t k = 0; k < n_kf; k++)
        if (kf_slot_start[k + 1] < kf_slot_start[k]) {
            err = std::string(name) + ": kf_slot_start decreases at keyframe " + std::to_string(k);
            return DEFTRI_E_ARG;
        }
    const int32_t n_slots = kf_slot_start[n_kf];
    for (int32_t s = 0; s < n_slots; s++)
        if (kf_octave[s] < 0 || kf_octave[s] >= n_scales) {
            err = std::string(name) + ": keypoint " + std::to_string(s) + " has octave " + std::to_string(kf_octave[s]) +
                  ", outside [0, nScales = " + std::to_string(n_scales) + ")";
            return DEFTRI_E_ARG;
        }
    for (int32_t p = 0; p < n; p++) {
        if (obs_start[p + 1] < obs_start[p]) {
            err = std::string(name) + ": obs_start decreases at map point " + std::to_string(p);
            return DEFTRI_E_ARG;
        }
        for (int32_t o = obs_start[p]; o < obs_start[p + 1]; o++) {
            const int32_t kf = obs_kf[o];
            if (kf < 0 || kf >= n_kf || obs_slot[o] < 0 || obs_slot[o] >= kf_slot_start[kf + 1] - kf_slot_start[kf]) {
                err = std::string(name) + ": observation " + std::to_string(o - obs_start[p]) + " of map point " + std::to_string(p) +
                      " names keyframe " + std::to_string(kf) + " slot " + std::to_string(obs_slot[o]) + ", which does not exist";
                return DEFTRI_E_ARG;
            }
        }
    }
    const int32_t n_obs = obs_start[n];
    const std::vector<float> scale = scale_table(n_scales, scale_factor);
    std::vector<float> centre(3 * (size_t)n_kf);
    for (int32_t k = 0; k < n_kf; k++) {
        float Ti[12];
        pose34_inverse(kf_Tcw + 12 * (size_t)k, Ti);
        centre[3 * k] = Ti[3]; centre[3 * k + 1] = Ti[7]; centre[3 * k + 2] = Ti[11];
    }
    auto ordinal_error = [&](int32_t p, int32_t ordinal) {
        err = std::string(name) + ": map point " + std::to_string(p) + ": the reference reads keypoint " + std::to_string(ordinal) +
              " (the chosen observation's ordinal, Map.cc:312) of keyframe " + std::to_string(obs_kf[obs_start[p] + ordinal]) +
              ", which has fewer slots";
        return DEFTRI_E_ARG;
    };

    if (device < 0) {
        std::vector<int> dists;
        for (int32_t p = 0; p < n; p++) {
            const int32_t o0 = obs_start[p], nobs = obs_start[p + 1] - o0;
            if (nobs == 0) {
                status[p] = 1;
                ref_obs[p] = -1;
                continue;
            }
            const V3 X = v3(pos[3 * p], pos[3 * p + 1], pos[3 * p + 2]);
            auto centre_of = [&](int32_t kf) { return v3(centre[3 * kf], centre[3 * kf + 1], centre[3 * kf + 2]); };
            auto desc_of = [&](int32_t i) { return kf_desc + 32 * ((size_t)kf_slot_start[obs_kf[o0 + i]] + obs_slot[o0 + i]); };
            V3 nsum = v3(0.0f, 0.0f, 0.0f);
            for (int32_t i = 0; i < nobs; i++) nsum = add(nsum, eigen_normalized(sub(X, centre_of(obs_kf[o0 + i]))));
            const float cnt = (float)nobs;
            const V3 nrml = eigen_normalized(v3(nsum.x / cnt, nsum.y / cnt, nsum.z / cnt));
            float best_median = 255.0f;
            int32_t obs_idx = 0;
            dists.resize((size_t)nobs);
            for (int32_t i = 0; i < nobs; i++) {
                for (int32_t j = 0; j < nobs; j++) dists[j] = hamming(desc_of(i), desc_of(j));
                std::nth_element(dists.begin(), dists.begin() + nobs / 2, dists.end());
                if ((float)dists[nobs / 2] < best_median) {
                    best_median = (float)dists[nobs / 2];
                    obs_idx = i;
                }
            }
            const int32_t kf = obs_kf[o0 + obs_idx];
            if (obs_idx >= kf_slot_start[kf + 1] - kf_slot_start[kf]) return ordinal_error(p, obs_idx);
            const float dist = nrm(sub(X, centre_of(kf)));
            const int ref_octave = kf_octave[kf_slot_start[kf] + obs_idx];
            const float mx = dist * scale[ref_octave];
            normal[3 * p] = nrml.x; normal[3 * p + 1] = nrml.y; normal[3 * p + 2] = nrml.z;
            max_dist[p] = mx;
            min_dist[p] = mx / scale[n_scales - 1];
            std::memcpy(desc + 32 * (size_t)p, desc_of(obs_idx), 32);
            ref_obs[p] = obs_idx;
            status[p] = 0;
        }
        return 0;
    }

    hipSetDevice(device);
    const size_t N = (size_t)n, NO = (size_t)n_obs, NK = (size_t)n_kf, NS = (size_t)n_slots;
    DevArena A;
    float *d_pos, *d_centre, *d_scale, *d_normal, *d_max, *d_min;
    int *d_obs_start, *d_obs_kf, *d_obs_slot, *d_kf_start, *d_kf_octave, *d_ref;
    uint4 *d_kf_desc, *d_desc;
    uint8_t *d_status;
    A.in(&d_pos, pos, 3 * N); A.in(&d_obs_start, obs_start, N + 1); A.in(&d_obs_kf, obs_kf, NO); A.in(&d_obs_slot, obs_slot, NO);
    A.in(&d_centre, centre.data(), 3 * NK); A.in(&d_kf_start, kf_slot_start, NK + 1); A.in(&d_kf_desc, kf_desc, 2 * NS);
    A.in(&d_kf_octave, kf_octave, NS); A.in(&d_scale, scale.data(), scale.size());
    A.add(&d_normal, 3 * N); A.add(&d_max, N); A.add(&d_min, N); A.add(&d_desc, 2 * N); A.add(&d_ref, N); A.add(&d_status, N);
    if (!A.commit(st)) {
        err = std::string(name) + ": allocation failed";
        return DEFTRI_E_HIP;
    }
    hipLaunchKernelGGL(dev::k_map_point_descriptors, dim3((n + 3) / 4), dim3(256), 0, st, n, d_pos, d_obs_start, d_obs_kf, d_obs_slot,
                       d_centre, d_kf_start, d_kf_desc, d_kf_octave, (int)n_scales, d_scale, d_normal, d_max, d_min, d_desc, d_ref,
                       d_status);
    // a point of status 1 or 2 leaves its outputs as the caller has them
    std::vector<float> h_normal(3 * N), h_max(N), h_min(N);
    std::vector<uint8_t> h_desc(32 * N);
    hipMemcpyAsync(h_normal.data(), d_normal, 12 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(h_max.data(), d_max, 4 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(h_min.data(), d_min, 4 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(h_desc.data(), d_desc, 32 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(ref_obs, d_ref, 4 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(status, d_status, N, hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(err, name, e);
    for (int32_t p = 0; p < n; p++) {
        if (status[p] == 2) return ordinal_error(p, ref_obs[p]);
        if (status[p] != 0) continue;
        std::memcpy(normal + 3 * (size_t)p, h_normal.data() + 3 * (size_t)p, 12);
        max_dist[p] = h_max[p];
        min_dist[p] = h_min[p];
        std::memcpy(desc + 32 * (size_t)p, h_desc.data() + 32 * (size_t)p, 32);
    }
    return 0;
}

}  // namespace deftri
