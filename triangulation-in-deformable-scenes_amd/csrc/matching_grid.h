// matching_grid.h — what the descriptor matchers share (matching.hip: searchForInitializaion;
// projection_matching.hip: guidedMatching, searchWithProjection): the Frame's feature grid as the
// reference reads it (Frame::posInGrid, Frame.cc:277-286; the cell range of getFeaturesInArea, :296-307),
// the acceptance test, the popcount Hamming distance, the (best, second, index) join of a wave and the
// window search itself, once for a wave (wave_window_best) and once as the reference's sequential loop
// (host_window_best).
// Float arithmetic, one rounding per operation: the including files are built without contraction.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/deftri.h"
#include "device_math.h"

namespace deftri {

namespace dev {
// Frame::initializeGrid / computeImageBoundaries (Frame.cc:213-227)
struct GridGeom {
    int cols, rows;
    float min_col, min_row, width_inv, height_inv;
};

inline GridGeom geometry(const deftri_feature_grid &g) {
    GridGeom G;
    G.cols = g.cols; G.rows = g.rows;
    G.min_col = g.min_col; G.min_row = g.min_row;
    G.width_inv = (float)g.cols / (float)(g.max_col - g.min_col);
    G.height_inv = (float)g.rows / (float)(g.max_row - g.min_row);
    return G;
}

// Frame::posInGrid (Frame.cc:277-286).  The reference converts the rounded float to int before it
// tests the range; a value no int holds (or a NaN) is outside the grid here as well.
__host__ __device__ __forceinline__ bool pos_in_grid(const GridGeom &G, float x, float y, int &col, int &row) {
    const float fc = roundf((x - G.min_col) * G.width_inv);
    const float fr = roundf((y - G.min_row) * G.height_inv);
    const bool ok = fc >= 0.0f && fc < (float)G.cols && fr >= 0.0f && fr < (float)G.rows;
    col = ok ? (int)fc : 0;
    row = ok ? (int)fr : 0;
    return ok;
}

// the cell range of Frame::getFeaturesInArea (Frame.cc:296-307): each of the four calls falls back when
// it fails, also when it fails through its other coordinate
__host__ __device__ __forceinline__ void cell_range(const GridGeom &G, float x, float y, float radius, int &cmin, int &rmin,
                                                    int &cmax, int &rmax) {
    int dummy;
    if (!pos_in_grid(G, x - radius, y, cmin, dummy)) cmin = 0;
    if (!pos_in_grid(G, x, y - radius, dummy, rmin)) rmin = 0;
    if (!pos_in_grid(G, x + radius, y, cmax, dummy)) cmax = G.cols - 1;
    if (!pos_in_grid(G, x, y + radius, dummy, rmax)) rmax = G.rows - 1;
}

// DescriptorMatching.cc:92, the literal expression
__host__ __device__ __forceinline__ bool accept_match(int best, int second, int th) {
    return best <= th && (double)(float)best < (double)(float)second * 0.9;
}

// Eigen's normalized(): the vector itself when its squared norm is not positive
__host__ __device__ __forceinline__ V3 eigen_normalized(V3 a) {
    const float z = dot(a, a);
    if (!(z > 0.0f)) return a;
    const float n = sqrtf(z);
    return v3(a.x / n, a.y / n, a.z / n);
}

// HammingDistance (DescriptorMatching.cc:21-36) of two 256-bit descriptors held as two uint4 each
__device__ __forceinline__ int hamming256(uint4 a0, uint4 a1, uint4 c0, uint4 c1) {
    const unsigned long long w0 = ((unsigned long long)(a0.y ^ c0.y) << 32) | (a0.x ^ c0.x);
    const unsigned long long w1 = ((unsigned long long)(a0.w ^ c0.w) << 32) | (a0.z ^ c0.z);
    const unsigned long long w2 = ((unsigned long long)(a1.y ^ c1.y) << 32) | (a1.x ^ c1.x);
    const unsigned long long w3 = ((unsigned long long)(a1.w ^ c1.w) << 32) | (a1.z ^ c1.z);
    return __popcll(w0) + __popcll(w1) + __popcll(w2) + __popcll(w3);
}

// (best, second, index) of two candidate sets joined: the two smallest distances of the union, the
// lower index among equal bests.  Identity (255, 255, -1).
__device__ __forceinline__ void join_best(int &b, int &s, int &idx, int b2, int s2, int idx2) {
    const int lo = min(b, b2), hi = max(b, b2);
    if (b2 < b || (b2 == b && idx2 >= 0 && (idx < 0 || idx2 < idx))) idx = idx2;
    s = min(hi, min(s, s2));
    b = lo;
}

// what a window search ends with: the two smallest distances (255 without a candidate), the best one's
// keypoint (-1 without one) and how many keypoints passed the octave and window tests, skipped ones included
struct WindowBest { int best, second, idx, ncand; };

// The window search of one 64-lane wave: the keypoints of getFeaturesInArea(x, y, radius, octave - 1,
// octave + 1) (Frame.cc:288-323) that `skip` does not pass over, against the descriptor (a0, a1).  A column
// of the cell range is one run of cell_keys (cells c * rows + rmin .. rmax are adjacent); the lanes stride
// over it.  The lowest index wins among equal bests.  The result is uniform across the wave.
template <typename Skip>
__device__ __forceinline__ WindowBest wave_window_best(const GridGeom &G, const int *__restrict__ cell_start,
                                                       const int *__restrict__ cell_keys, const float *__restrict__ uv2,
                                                       const int *__restrict__ octave2, const uint4 *__restrict__ desc2, float x,
                                                       float y, float radius, int octave, uint4 a0, uint4 a1, int lane, Skip skip) {
    const int min_level = octave - 1, max_level = octave + 1;             // DescriptorMatching.cc:72
    int b = 255, s = 255, idx = -1, ncand = 0;
    int cmin, rmin, cmax, rmax;
    cell_range(G, x, y, radius, cmin, rmin, cmax, rmax);
    for (int c = cmin; c <= cmax; c++) {
        if (rmin > rmax) break;
        const int k0 = cell_start[c * G.rows + rmin], k1 = cell_start[c * G.rows + rmax + 1];
        for (int k = k0 + lane; k < k1; k += 64) {
            const int j = cell_keys[k];
            const int o = octave2[j];
            if (o < min_level || o > max_level) continue;                       // Frame.cc:315
            const float dx = uv2[2 * j] - x, dy = uv2[2 * j + 1] - y;
            if (!(fabsf(dx) < radius && fabsf(dy) < radius)) continue;          // :317
            ncand++;
            if (skip(j)) continue;
            const int d = hamming256(a0, a1, desc2[2 * (size_t)j], desc2[2 * (size_t)j + 1]);
            // DescriptorMatching.cc:82-89; a distance of 255 or 256 changes nothing
            if (d < b) { s = b; b = d; idx = j; }
            else {
                if (d < s) s = d;
                if (d == b && d < 255 && j < idx) idx = j;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int b2 = __shfl_xor(b, off, 64), s2 = __shfl_xor(s, off, 64), i2 = __shfl_xor(idx, off, 64);
        join_best(b, s, idx, b2, s2, i2);
        ncand += __shfl_xor(ncand, off, 64);
    }
    return {b, s, idx, ncand};
}
}  // namespace dev

// ---- host helpers of both matchers (defined in matching.hip) ----
// "" for a grid Frame could have built, else what is wrong with it
std::string grid_error(const deftri_feature_grid &g);
// getScaleFactor(octave) of Frame's table (Frame.cc:65-70): a running float product
float scale_factor(const deftri_feature_grid &g, int octave);
// the reference reads vScaleFactor_[octave]: true when octave[i] is in [0, nScales) for every i (of those with
// has[i] when `has` is given), else "<entry>: <what> i has octave ..." in err
bool octaves_ok(const char *entry, const char *what, const deftri_feature_grid &g, int32_t n, const int32_t *octave,
                const uint8_t *has, std::string &err);
// cell_start / cell_keys of `uv` on the device (k_grid_cells / k_excl_scan / k_grid_fill on `st`): d_cell
// [n], d_count / d_cursor [ncell], d_start [ncell + 1], d_keys [n]; ncell = cols * rows
void launch_grid(const dev::GridGeom &G, int n, const float *d_uv, int *d_cell, int *d_count, int *d_start, int *d_cursor,
                 int *d_keys, hipStream_t st);
// its second half for a caller that wrote d_cell and d_count (zeroed first) itself: k_excl_scan / k_grid_fill
void launch_grid_lists(int ncell, int n, const int *d_cell, const int *d_count, int *d_start, int *d_cursor, int *d_keys,
                       hipStream_t st);
// d_keys' runs in keypoint order into d_ordered [n], as the reference's push_back leaves them (k_grid_order)
void launch_grid_order(int n, const int *d_cell, const int *d_start, const int *d_keys, int *d_ordered, hipStream_t st);
// Frame::distributeFeatures' grid (Frame.cc:204-210) on the host: grid[c * rows + r] in keypoint order
std::vector<std::vector<int32_t>> host_grid(const dev::GridGeom &G, int32_t n, const float *uv);
// HammingDistance (DescriptorMatching.cc:21-36) over 8 32-bit words
int hamming(const uint8_t *a, const uint8_t *b);

// The window search as the reference runs it: getFeaturesInArea over host_grid's cells (columns, then rows,
// then keys in keypoint order), then the two-smallest loop (DescriptorMatching.cc:76-90) over the keys that
// `skip` does not pass over, against the 32-byte descriptor `desc`.  The first key visited wins among equal bests.
template <typename Skip>
dev::WindowBest host_window_best(const dev::GridGeom &G, const std::vector<std::vector<int32_t>> &cells, const float *uv2,
                                 const int32_t *octave2, const uint8_t *desc2, float x, float y, float radius, int octave,
                                 const uint8_t *desc, Skip skip) {
    dev::WindowBest w{255, 255, -1, 0};
    int cmin, rmin, cmax, rmax;
    dev::cell_range(G, x, y, radius, cmin, rmin, cmax, rmax);
    for (int c = cmin; c <= cmax; c++)
        for (int r = rmin; r <= rmax; r++)
            for (int32_t j : cells[(size_t)c * G.rows + r]) {
                const int o = octave2[j];
                if (o < octave - 1 || o > octave + 1) continue;                     // Frame.cc:315
                const float dx = uv2[2 * j] - x, dy = uv2[2 * j + 1] - y;
                if (!(fabsf(dx) < radius && fabsf(dy) < radius)) continue;          // :317
                w.ncand++;
                if (skip(j)) continue;
                const int dist = hamming(desc, desc2 + 32 * (size_t)j);
                if (dist < w.best) {
                    w.second = w.best;
                    w.best = dist;
                    w.idx = j;
                } else if (dist < w.second) {
                    w.second = dist;
                }
            }
    return w;
}

}  // namespace deftri
