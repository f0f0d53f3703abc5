// undistort.hip — from the distorted keypoints FAST::extract leaves to the frame the matchers read: the third line
// of Mapping::extractFeatures (Mapping.cc:120-129), currFrame_.distributeFeatures().
//
// With Camera.k1 the reference undistorts every keypoint slot with cv::undistortPoints (Frame::undistortKeys,
// Frame.cc:252-275) and Frame's constructor undistorts the four image corners into the grid bounds
// (computeImageBoundaries, :221-250); then distributeFeatures (:190-211) pushes every slot whose own posInGrid
// succeeds into grid_[col][row].  cv::undistortPoints is restated from its definition (undistort.h); it has
// not been run against an OpenCV build.
//   k_undistort            one thread per point (deftri_undistort_points)
//   k_undistort_cells      one thread per slot: the undistorted key, its cell, in_grid and the cell's count
//   then k_excl_scan (dev_scan.h) and matching.hip's k_grid_fill / k_grid_order: the lists as a CSR in keypoint order
// The four corners are undistorted on the host on both contexts, by the same function: the kernels take the
// grid geometry by value.  The keys stay on the device between undistortion and grid.
//
// Double arithmetic for the undistortion, float for posInGrid, both without contraction on host and device;
// the host loops below are the sequential restatements a host-only context runs and the kernels are tested
// against, bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "dev_arena.h"
#include "matching_grid.h"
#include "undistort.h"

namespace deftri {

namespace dev {
// in place where uv_in == uv_out: a thread reads its point before it writes it
__global__ void k_undistort(int n, const float2 *uv_in, UndistortModel M, float2 *uv_out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const float2 p = uv_in[i];
    float2 o;
    undistort_point(M, p.x, p.y, o.x, o.y);
    uv_out[i] = o;
}

// Frame::undistortKeys and the first half of distributeFeatures' loop for slot i: `count` zeroed before
__global__ void k_undistort_cells(int n, const float2 *__restrict__ uv_dis, int undistort, UndistortModel M, GridGeom G,
                                  float2 *__restrict__ uv, int *__restrict__ cell, uint8_t *__restrict__ in_grid,
                                  int *__restrict__ count) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    float2 p = uv_dis[i];
    if (undistort) undistort_point(M, p.x, p.y, p.x, p.y);
    uv[i] = p;
    int c, r;
    const bool in = pos_in_grid(G, p.x, p.y, c, r);
    const int id = in ? c * G.rows + r : -1;
    cell[i] = id;
    in_grid[i] = in ? 1 : 0;
    if (in) atomicAdd(&count[id], 1);
}
}  // namespace dev

using namespace dev;

namespace {
// "" and the model, or what is wrong with the arguments
std::string model_of(const float *calib, const float *dist, int32_t n_dist, UndistortModel &M) {
    if (n_dist != 0 && n_dist != 4 && n_dist != 5) return "n_dist = " + std::to_string(n_dist) + ", not 0, 4 or 5";
    std::memset(&M, 0, sizeof(M));
    if (n_dist == 0) return "";
    if (!calib || !dist) return "null calib or dist with n_dist > 0";
    if (!std::isfinite(calib[0]) || !std::isfinite(calib[1]) || calib[0] == 0.0f || calib[1] == 0.0f)
        return "Camera.fx or Camera.fy is zero or not finite: the undistortion divides by them";
    M.fx = calib[0]; M.fy = calib[1]; M.cx = calib[2]; M.cy = calib[3];
    M.k1 = dist[0]; M.k2 = dist[1]; M.p1 = dist[2]; M.p2 = dist[3];
    M.k3 = n_dist == 5 ? (double)dist[4] : 0.0;
    return "";
}

// Frame::computeImageBoundaries (Frame.cc:221-250)
void bounds_of(const UndistortModel &M, int32_t n_dist, int32_t cols, int32_t rows, float *b) {
    const float fc = (float)cols, fr = (float)rows;
    if (n_dist == 0) {
        b[0] = 0.0f; b[1] = 0.0f; b[2] = fc; b[3] = fr;
        return;
    }
    const float corners[8] = {0.0f, 0.0f, fc, 0.0f, 0.0f, fr, fc, fr};
    float o[8];
    for (int k = 0; k < 4; k++) undistort_point(M, corners[2 * k], corners[2 * k + 1], o[2 * k], o[2 * k + 1]);
    b[0] = std::min(o[0], o[4]);    // minCol_ = min(o0.x, o2.x)
    b[1] = std::min(o[1], o[3]);    // minRow_ = min(o0.y, o1.y)
    b[2] = std::max(o[2], o[6]);    // maxCol_ = max(o1.x, o3.x)
    b[3] = std::max(o[5], o[7]);    // maxRow_ = max(o2.y, o3.y)
}
}  // namespace

int undistort_points(int device, hipStream_t st, int32_t n, const float *uv_in, const float *calib, const float *dist,
                     int32_t n_dist, float *uv_out, std::string &err) {
    UndistortModel M;
    if (n_dist == 0) {
        err = "undistort_points: n_dist = 0, not 4 or 5";
        return DEFTRI_E_ARG;
    }
    const std::string why = model_of(calib, dist, n_dist, M);
    if (!why.empty()) {
        err = "undistort_points: " + why;
        return DEFTRI_E_ARG;
    }
    if (n == 0) return 0;
    if (device < 0) {
        for (int32_t i = 0; i < n; i++) {
            const float u = uv_in[2 * i], v = uv_in[2 * i + 1];
            undistort_point(M, u, v, uv_out[2 * i], uv_out[2 * i + 1]);
        }
        return 0;
    }
    hipSetDevice(device);
    const size_t N = (size_t)n;
    DevArena A;
    float2 *d_uv;
    A.in(&d_uv, uv_in, N);
    if (!A.commit(st)) {
        err = "undistort_points: allocation failed";
        return DEFTRI_E_HIP;
    }
    hipLaunchKernelGGL(dev::k_undistort, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, n, d_uv, M, d_uv);
    hipMemcpyAsync(uv_out, d_uv, 8 * N, hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(err, "undistort_points", e);
    return 0;
}

int image_bounds(int32_t cols, int32_t rows, const float *calib, const float *dist, int32_t n_dist, float *bounds,
                 std::string &err) {
    UndistortModel M;
    const std::string why = model_of(calib, dist, n_dist, M);
    if (!why.empty()) {
        err = "image_bounds: " + why;
        return DEFTRI_E_ARG;
    }
    float b[4];
    bounds_of(M, n_dist, cols, rows, b);
    if (!(b[2] > b[0]) || !(b[3] > b[1])) {
        err = "image_bounds: max <= min after undistortion";
        return DEFTRI_E_ARG;
    }
    std::memcpy(bounds, b, sizeof(b));
    return 0;
}

int distribute_features(int device, hipStream_t st, int32_t grid_cols, int32_t grid_rows, int32_t n_scales, float scale_factor,
                        int32_t cols, int32_t rows, const float *calib, const float *dist, int32_t n_dist, int32_t n,
                        const float *uv_dis, float *uv, deftri_feature_grid *grid, int32_t *cell_start, int32_t *cell_items,
                        uint8_t *in_grid, std::string &err) {
    UndistortModel M;
    std::string why = model_of(calib, dist, n_dist, M);
    deftri_feature_grid g{};
    if (why.empty()) {
        float b[4];
        bounds_of(M, n_dist, cols, rows, b);
        g.cols = grid_cols; g.rows = grid_rows;
        g.min_col = b[0]; g.min_row = b[1]; g.max_col = b[2]; g.max_row = b[3];
        g.n_scales = n_scales; g.scale_factor = scale_factor;
        why = grid_error(g);
        if (why == "feature grid bounds: max <= min") why += " after undistortion";
    }
    if (!why.empty()) {
        err = "distribute_features: " + why;
        return DEFTRI_E_ARG;
    }
    const GridGeom G = geometry(g);
    const size_t ncell = (size_t)G.cols * G.rows, N = (size_t)n;
    *grid = g;
    if (device < 0 || n == 0) {
        // Frame::undistortKeys over every slot, then distributeFeatures' loop (Frame.cc:204-210)
        for (int32_t i = 0; i < n; i++) {
            float x = uv_dis[2 * i], y = uv_dis[2 * i + 1];
            if (n_dist) undistort_point(M, x, y, x, y);
            uv[2 * i] = x;
            uv[2 * i + 1] = y;
            if (in_grid) {
                int c, r;
                in_grid[i] = pos_in_grid(G, x, y, c, r) ? 1 : 0;
            }
        }
        const auto cells = host_grid(G, n, uv);
        int32_t run = 0;
        for (size_t c = 0; c < ncell; c++) {
            cell_start[c] = run;
            for (int32_t k : cells[c]) cell_items[run++] = k;
        }
        cell_start[ncell] = run;
        for (int32_t k = run; k < n; k++) cell_items[k] = -1;
        return 0;
    }
    hipSetDevice(device);
    DevArena A;
    float2 *d_dis, *d_uv;
    int *d_cell, *d_keys, *d_ordered, *d_count, *d_cursor, *d_start;
    uint8_t *d_in;
    A.in(&d_dis, uv_dis, N); A.add(&d_uv, N);
    A.add(&d_cell, N); A.add(&d_keys, N); A.add(&d_ordered, N); A.add(&d_count, ncell); A.add(&d_cursor, ncell);
    A.add(&d_start, ncell + 1); A.add(&d_in, N);
    if (!A.commit(st)) {
        err = "distribute_features: allocation failed";
        return DEFTRI_E_HIP;
    }
    hipMemsetAsync(d_count, 0, sizeof(int) * ncell, st);
    hipMemsetAsync(d_ordered, 0xff, sizeof(int) * N, st);   // -1 behind the keys that are in the grid
    hipLaunchKernelGGL(dev::k_undistort_cells, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, n, d_dis, n_dist ? 1 : 0, M, G,
                       d_uv, d_cell, d_in, d_count);
    launch_grid_lists((int)ncell, n, d_cell, d_count, d_start, d_cursor, d_keys, st);
    launch_grid_order(n, d_cell, d_start, d_keys, d_ordered, st);
    hipMemcpyAsync(uv, d_uv, 8 * N, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(cell_start, d_start, 4 * (ncell + 1), hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(cell_items, d_ordered, 4 * N, hipMemcpyDeviceToHost, st);
    if (in_grid) hipMemcpyAsync(in_grid, d_in, N, hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(err, "distribute_features", e);
    return 0;
}

}  // namespace deftri
