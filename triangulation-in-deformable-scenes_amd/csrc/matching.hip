// matching.hip — from two frames' keypoints to the correspondences reconstructPoints takes.
//
// searchForInitializaion (reference Modules/Matching/DescriptorMatching.cc:39-99): for every reference
// keypoint of octave <= 0, the current frame's keypoints in a window of its feature grid
// (Frame::getFeaturesInArea, Frame.cc:288-323, over Frame::posInGrid, :277-286), the two smallest Hamming
// distances among them (both start at 255), and the acceptance bestDist <= th && (float)bestDist <
// float(secondBestDist) * 0.9.  (best, second) are the two smallest of a multiset, so the order the
// candidates are visited in does not change them, and an accepted best is strictly below the second:
// its index is unique.  The device therefore reduces in any order and equals the sequential loop.
//   k_grid_cells / k_excl_scan / k_grid_fill   the current frame's cell lists as a CSR (the scan: dev_scan.h)
//   k_grid_order                               the lists in keypoint order (undistort.hip's distributeFeatures)
//   k_match_init                               one 64-lane wave per reference keypoint (wave_window_best)
//   k_count_matches                            nMatches
// posInGrid rounds to the nearest cell index, so a keypoint in the last half cell of the image gets
// index == size, is in no cell (Frame.cc:204-210) and is never a candidate: kept.
//
// The epipolar mask of MonocularMapInitializer::initialize with Triangulation.checks
// (MonocularMapInitializer.cc:93-104): findEssentialWithRANSAC (:119-178) scores the same E, built from
// the poses (:160-163), in every iteration, so its result is one computeScoreAndInliers (:206-223):
//   k_epipolar_inliers                         one thread per match, the score per workgroup
//
// The grid geometry, the acceptance test and the window search of a wave and of the host loop are in
// matching_grid.h, shared with projection_matching.hip.
//
// Float arithmetic without contraction on both sides; the host loops below are the sequential
// restatements a host-only context runs and the kernels are tested against.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "dev_arena.h"
#include "dev_scan.h"
#include "device_math.h"
#include "epipolar.h"
#include "matching.h"
#include "matching_grid.h"
#include "pose_host.h"

namespace deftri {

namespace dev {
// epipolar_error (computeScoreAndInliers for one match) is in epipolar.h, shared with essential.hip

// the cell of every keypoint (c * rows + r, -1 outside the grid) and the cells' sizes
__global__ void k_grid_cells(int n, const float *__restrict__ uv, GridGeom G, int *__restrict__ cell, int *__restrict__ count) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    int c, r;
    const bool in = pos_in_grid(G, uv[2 * i], uv[2 * i + 1], c, r);
    const int id = in ? c * G.rows + r : -1;
    cell[i] = id;
    if (in) atomicAdd(&count[id], 1);
}

// the cell lists from the scanned sizes; cursor [ncell] = start on entry (k_excl_scan's second output)
__global__ void k_grid_fill(int n, const int *__restrict__ cell, int *__restrict__ cursor, int *__restrict__ keys) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int id = cell[i];
    if (id >= 0) keys[atomicAdd(&cursor[id], 1)] = i;
}

// the filled lists put into keypoint order, as the reference's push_back leaves them: keypoint i goes to the
// place in its cell's run given by how many of the run's keys are below it.  `keys` is read, `ordered` written.
__global__ void k_grid_order(int n, const int *__restrict__ cell, const int *__restrict__ start, const int *__restrict__ keys,
                             int *__restrict__ ordered) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int id = cell[i];
    if (id < 0) return;
    const int k0 = start[id], k1 = start[id + 1];
    int below = 0;
    for (int k = k0; k < k1; k++) below += keys[k] < i ? 1 : 0;
    ordered[k0 + below] = i;
}

// One wave per reference keypoint (4 per workgroup).  `radius`: windowSizeFactor * 1 * getScaleFactor(0),
// the only octave searched (:56).
__global__ void __launch_bounds__(256)
k_match_init(int n1, const float *__restrict__ uv1, const int *__restrict__ octave1, const uint4 *__restrict__ desc1,
             const float *__restrict__ uv2, const int *__restrict__ octave2, const uint4 *__restrict__ desc2, GridGeom G,
             const int *__restrict__ cell_start, const int *__restrict__ cell_keys, float radius, int th,
             int *__restrict__ matches, int *__restrict__ best_out, int *__restrict__ second_out) {
    const int lane = threadIdx.x & 63;
    const int i = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (i >= n1) return;
    const int oct = octave1[i];
    WindowBest w{255, 255, -1, 0};
    if (oct <= 0)                                                      // :56
        w = wave_window_best(G, cell_start, cell_keys, uv2, octave2, desc2, uv1[2 * i], uv1[2 * i + 1], radius, oct,
                             desc1[2 * (size_t)i], desc1[2 * (size_t)i + 1], lane, [](int) { return false; });
    if (lane == 0) {
        matches[i] = (oct <= 0 && accept_match(w.best, w.second, th)) ? w.idx : -1;   // :92-95
        best_out[i] = w.best;
        second_out[i] = w.second;
    }
}

__global__ void k_count_matches(int n, const int *__restrict__ matches, int *__restrict__ total) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const unsigned long long m = __ballot(i < n && matches[i] >= 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(total, __popcll(m));
}

// part [gridDim.x]: the inliers of each workgroup (a ballot per wave, then the four waves); the host
// adds them in workgroup order
__global__ void __launch_bounds__(256)
k_epipolar_inliers(int n, const float *__restrict__ uv1, const float *__restrict__ uv2, Kb8 k1, Kb8 k2, Mat3 E, float th,
                   uint8_t *__restrict__ inlier, float *__restrict__ err, int *__restrict__ part) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    bool in = false;
    if (i < n) {
        const float e = epipolar_error(k1, k2, E, uv1[2 * i], uv1[2 * i + 1], uv2[2 * i], uv2[2 * i + 1]);
        in = e < th;                                                   // :211
        inlier[i] = in ? 1 : 0;
        err[i] = e;
    }
    __shared__ int red[4];
    const unsigned long long m = __ballot(in);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace dev

using namespace dev;

// "" for a grid Frame could have built, else what is wrong with it
std::string grid_error(const deftri_feature_grid &g) {
    if (g.cols <= 0 || g.rows <= 0) return "FeatureGrid.nGridCols / nGridRows must be positive";
    if ((int64_t)g.cols * g.rows > ((int64_t)1 << 24)) return "feature grid of more than 2^24 cells";
    if (!(g.max_col > g.min_col) || !(g.max_row > g.min_row)) return "feature grid bounds: max <= min";
    if (g.n_scales < 1) return "FeatureExtractor.nScales < 1";
    return "";
}

// the reference reads vScaleFactor_[octave] of the keypoint (DescriptorMatching.cc:69)
bool octaves_ok(const char *entry, const char *what, const deftri_feature_grid &g, int32_t n, const int32_t *octave,
                const uint8_t *has, std::string &err) {
    for (int32_t i = 0; i < n; i++)
        if ((!has || has[i]) && (octave[i] < 0 || octave[i] >= g.n_scales)) {
            err = std::string(entry) + ": " + what + " " + std::to_string(i) + " has octave " + std::to_string(octave[i]) +
                  ", outside [0, nScales = " + std::to_string(g.n_scales) + ")";
            return false;
        }
    return true;
}

// getScaleFactor(octave) of Frame's table (Frame.cc:65-70): a running float product
float scale_factor(const deftri_feature_grid &g, int octave) {
    float s = 1.0f;
    for (int i = 1; i <= octave; i++) s = s * g.scale_factor;
    return s;
}

// cell_start / cell_keys of `uv` on the device (the arrays stay in A); ncell = cols * rows
void launch_grid(const GridGeom &G, int n, const float *d_uv, int *d_cell, int *d_count, int *d_start, int *d_cursor,
                 int *d_keys, hipStream_t st) {
    const int ncell = G.cols * G.rows;
    hipMemsetAsync(d_count, 0, sizeof(int) * (size_t)ncell, st);
    hipLaunchKernelGGL(dev::k_grid_cells, dim3((n + 255) / 256), dim3(256), 0, st, n, d_uv, G, d_cell, d_count);
    launch_grid_lists(ncell, n, d_cell, d_count, d_start, d_cursor, d_keys, st);
}

// the lists from every keypoint's cell and the cells' sizes: the scan and the fill
void launch_grid_lists(int ncell, int n, const int *d_cell, const int *d_count, int *d_start, int *d_cursor, int *d_keys,
                       hipStream_t st) {
    launch_excl_scan<int, 256>(ncell, d_count, d_start, d_cursor, st);
    hipLaunchKernelGGL(dev::k_grid_fill, dim3((n + 255) / 256), dim3(256), 0, st, n, d_cell, d_cursor, d_keys);
}

// d_keys' runs in keypoint order into d_ordered [n]
void launch_grid_order(int n, const int *d_cell, const int *d_start, const int *d_keys, int *d_ordered, hipStream_t st) {
    hipLaunchKernelGGL(dev::k_grid_order, dim3((n + 255) / 256), dim3(256), 0, st, n, d_cell, d_start, d_keys, d_ordered);
}

// Frame::distributeFeatures' grid (Frame.cc:204-210) on the host: grid[c * rows + r] in keypoint order
std::vector<std::vector<int32_t>> host_grid(const GridGeom &G, int32_t n, const float *uv) {
    std::vector<std::vector<int32_t>> grid((size_t)G.cols * G.rows);
    for (int32_t i = 0; i < n; i++) {
        int c, r;
        if (pos_in_grid(G, uv[2 * i], uv[2 * i + 1], c, r)) grid[(size_t)c * G.rows + r].push_back(i);
    }
    return grid;
}

// HammingDistance (DescriptorMatching.cc:21-36) over 8 32-bit words
int hamming(const uint8_t *a, const uint8_t *b) {
    int dist = 0;
    for (int w = 0; w < 8; w++) {
        uint32_t x, y;
        std::memcpy(&x, a + 4 * w, 4);
        std::memcpy(&y, b + 4 * w, 4);
        dist += __builtin_popcount(x ^ y);
    }
    return dist;
}

int feature_grid_cells(int device, hipStream_t st, const deftri_feature_grid &grid, int32_t n, const float *uv,
                       int32_t *cell_start, int32_t *cell_keys, std::string &err) {
    const std::string why = grid_error(grid);
    if (!why.empty()) {
        err = "feature_grid_cells: " + why;
        return DEFTRI_E_ARG;
    }
    const GridGeom G = geometry(grid);
    const size_t ncell = (size_t)G.cols * G.rows, N = (size_t)n;
    if (device < 0 || n == 0) {
        const auto cells = host_grid(G, n, uv);
        int32_t run = 0;
        for (size_t c = 0; c < ncell; c++) {
            cell_start[c] = run;
            for (int32_t k : cells[c]) cell_keys[run++] = k;
        }
        cell_start[ncell] = run;
        return 0;
    }
    hipSetDevice(device);
    DevArena A;
    float *d_uv;
    int *d_cell, *d_keys, *d_count, *d_cursor, *d_start;
    A.in(&d_uv, uv, 2 * N);
    A.add(&d_cell, N); A.add(&d_keys, N); A.add(&d_count, ncell); A.add(&d_cursor, ncell); A.add(&d_start, ncell + 1);
    if (!A.commit(st)) {
        err = "feature_grid_cells: allocation failed";
        return DEFTRI_E_HIP;
    }
    launch_grid(G, n, d_uv, d_cell, d_count, d_start, d_cursor, d_keys, st);
    hipMemcpyAsync(cell_start, d_start, 4 * (ncell + 1), hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(err, "feature_grid_cells", e);
    // only the filled part of cell_keys is defined
    const hipError_t e2 = hipMemcpy(cell_keys, d_keys, 4 * (size_t)cell_start[ncell], hipMemcpyDeviceToHost);
    if (e2 != hipSuccess) return hip_fail(err, "feature_grid_cells", e2);
    return 0;
}

int match_for_initialization(int device, hipStream_t st, const deftri_feature_grid &grid, int32_t n1, const float *uv1,
                             const int32_t *octave1, const uint8_t *desc1, int32_t n2, const float *uv2,
                             const int32_t *octave2, const uint8_t *desc2, int32_t th, float window_size_factor,
                             int32_t *matches, int32_t *best_dist, int32_t *second_dist, int32_t *n_matches,
                             std::string &err) {
    const char *name = "match_for_initialization";
    const std::string why = grid_error(grid);
    if (!why.empty()) {
        err = std::string(name) + ": " + why;
        return DEFTRI_E_ARG;
    }
    if (!octaves_ok(name, "reference keypoint", grid, n1, octave1, nullptr, err) ||
        !octaves_ok(name, "current keypoint", grid, n2, octave2, nullptr, err))
        return DEFTRI_E_ARG;
    const GridGeom G = geometry(grid);
    const float radius = window_size_factor * 1 * scale_factor(grid, 0);   // :69, octave 0 (the only one searched)
    *n_matches = 0;
    if (n1 == 0 || n2 == 0) {
        for (int32_t i = 0; i < n1; i++) {
            matches[i] = -1;
            if (best_dist) best_dist[i] = 255;
            if (second_dist) second_dist[i] = 255;
        }
        return 0;
    }
    if (device < 0) {
        const auto cells = host_grid(G, n2, uv2);
        int nm = 0;
        for (int32_t i = 0; i < n1; i++) {
            matches[i] = -1;                                           // :40
            if (best_dist) best_dist[i] = 255;
            if (second_dist) second_dist[i] = 255;
            if (octave1[i] > 0) continue;                              // :56
            const int last_octave = octave1[i];
            const float rad = window_size_factor * 1 * scale_factor(grid, last_octave);
            const WindowBest w = host_window_best(G, cells, uv2, octave2, desc2, uv1[2 * i], uv1[2 * i + 1], rad, last_octave,
                                                  desc1 + 32 * (size_t)i, [](int32_t) { return false; });
            if (accept_match(w.best, w.second, th)) {                  // :92-95
                matches[i] = w.idx;
                nm++;
            }
            if (best_dist) best_dist[i] = w.best;
            if (second_dist) second_dist[i] = w.second;
        }
        *n_matches = nm;
        return 0;
    }
    hipSetDevice(device);
    const size_t N1 = (size_t)n1, N2 = (size_t)n2, ncell = (size_t)G.cols * G.rows;
    DevArena A;
    float *d_uv1, *d_uv2;
    int *d_oct1, *d_oct2, *d_cell, *d_keys, *d_count, *d_cursor, *d_start, *d_match, *d_best, *d_second, *d_total;
    uint4 *d_desc1, *d_desc2;
    A.in(&d_uv1, uv1, 2 * N1); A.in(&d_oct1, octave1, N1); A.in(&d_desc1, desc1, 2 * N1);
    A.in(&d_uv2, uv2, 2 * N2); A.in(&d_oct2, octave2, N2); A.in(&d_desc2, desc2, 2 * N2);
    A.add(&d_cell, N2); A.add(&d_keys, N2); A.add(&d_count, ncell); A.add(&d_cursor, ncell); A.add(&d_start, ncell + 1);
    A.add(&d_match, N1); A.add(&d_best, N1); A.add(&d_second, N1); A.add(&d_total, 1);
    if (!A.commit(st)) {
        err = "match_for_initialization: allocation failed";
        return DEFTRI_E_HIP;
    }
    hipMemsetAsync(d_total, 0, sizeof(int), st);
    launch_grid(G, n2, d_uv2, d_cell, d_count, d_start, d_cursor, d_keys, st);
    hipLaunchKernelGGL(dev::k_match_init, dim3((n1 + 3) / 4), dim3(256), 0, st, n1, d_uv1, d_oct1, d_desc1, d_uv2, d_oct2,
                       d_desc2, G, d_start, d_keys, radius, th, d_match, d_best, d_second);
    hipLaunchKernelGGL(dev::k_count_matches, dim3((n1 + 255) / 256), dim3(256), 0, st, n1, d_match, d_total);
    int total = 0;
    hipMemcpyAsync(matches, d_match, 4 * N1, hipMemcpyDeviceToHost, st);
    if (best_dist) hipMemcpyAsync(best_dist, d_best, 4 * N1, hipMemcpyDeviceToHost, st);
    if (second_dist) hipMemcpyAsync(second_dist, d_second, 4 * N1, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(&total, d_total, sizeof(int), hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(err, "match_for_initialization", e);
    *n_matches = total;
    return 0;
}

int epipolar_inliers(int device, hipStream_t st, int32_t n, const float *uv1, const float *uv2, const float *kb8_1,
                     const float *kb8_2, const float *T1w, const float *T2w, float epipolar_th, uint8_t *inlier, float *err_out,
                     int32_t *score, std::string &err) {
    // T12 = T1w * T2w.inverse() (:162) and E = [t]x R (Geometry.cc:239-256), in float; poses row-major 3x4
    float T2i[12], T12[12];
    pose34_inverse(T2w, T2i);
    pose34_product(T1w, T2i, T12);
    const float t[3] = {T12[3], T12[7], T12[11]};
    const float tx[9] = {0.0f, -t[2], t[1], t[2], 0.0f, -t[0], -t[1], t[0], 0.0f};
    Mat3 E;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) E.m[3 * i + j] = tx[3 * i] * T12[j] + tx[3 * i + 1] * T12[4 + j] + tx[3 * i + 2] * T12[8 + j];
    Kb8 k1, k2;
    std::memcpy(k1.k, kb8_1, sizeof(k1.k));
    std::memcpy(k2.k, kb8_2, sizeof(k2.k));
    if (device < 0) {
        int sc = 0;
        for (int32_t i = 0; i < n; i++) {
            const float e = epipolar_error(k1, k2, E, uv1[2 * i], uv1[2 * i + 1], uv2[2 * i], uv2[2 * i + 1]);
            inlier[i] = e < epipolar_th ? 1 : 0;
            if (inlier[i]) sc++;
            if (err_out) err_out[i] = e;
        }
        *score = sc;
        return 0;
    }
    hipSetDevice(device);
    const size_t N = (size_t)n, nb = (N + 255) / 256;
    DevArena A;
    float *d_uv1, *d_uv2, *d_err;
    uint8_t *d_in;
    int *d_part;
    A.in(&d_uv1, uv1, 2 * N); A.in(&d_uv2, uv2, 2 * N); A.add(&d_in, N); A.add(&d_err, N); A.add(&d_part, nb);
    if (!A.commit(st)) {
        err = "epipolar_inliers: allocation failed";
        return DEFTRI_E_HIP;
    }
    std::vector<int> part(nb);
    hipLaunchKernelGGL(dev::k_epipolar_inliers, dim3((unsigned)nb), dim3(256), 0, st, n, d_uv1, d_uv2, k1, k2, E, epipolar_th,
                       d_in, d_err, d_part);
    hipMemcpyAsync(inlier, d_in, N, hipMemcpyDeviceToHost, st);
    if (err_out) hipMemcpyAsync(err_out, d_err, 4 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(part.data(), d_part, 4 * nb, hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(err, "epipolar_inliers", e);
    int sc = 0;
    for (size_t b = 0; b < nb; b++) sc += part[b];                     // workgroup order
    *score = sc;
    return 0;
}

}  // namespace deftri
