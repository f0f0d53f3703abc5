// matching_grid.h — what the descriptor matchers share (matching.hip: searchForInitializaion;
// projection_matching.hip: guidedMatching, searchWithProjection): the Frame's feature grid as the
// reference reads it (Frame::posInGrid, Frame.cc:277-286; the cell range of getFeaturesInArea, :296-307),
// the acceptance test, the popcount Hamming distance and the (best, second, index) join of a wave.
// Float arithmetic, one rounding per operation: the including files are built without contraction.
#pragma once
#include <hip/hip_runtime.h>

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
}  // namespace dev

// ---- host helpers of both matchers (defined in matching.hip) ----
// "" for a grid Frame could have built, else what is wrong with it
std::string grid_error(const deftri_feature_grid &g);
// getScaleFactor(octave) of Frame's table (Frame.cc:65-70): a running float product
float scale_factor(const deftri_feature_grid &g, int octave);
// cell_start / cell_keys of `uv` on the device (k_grid_cells / k_grid_scan / k_grid_fill on `st`): d_cell
// [n], d_count / d_cursor [ncell], d_start [ncell + 1], d_keys [n]; ncell = cols * rows
void launch_grid(const dev::GridGeom &G, int n, const float *d_uv, int *d_cell, int *d_count, int *d_start, int *d_cursor,
                 int *d_keys, hipStream_t st);
// its second half for a caller that wrote d_cell and d_count (zeroed first) itself: k_grid_scan / k_grid_fill
void launch_grid_lists(int ncell, int n, const int *d_cell, const int *d_count, int *d_start, int *d_cursor, int *d_keys,
                       hipStream_t st);
// d_keys' runs in keypoint order into d_ordered [n], as the reference's push_back leaves them (k_grid_order)
void launch_grid_order(int n, const int *d_cell, const int *d_start, const int *d_keys, int *d_ordered, hipStream_t st);
// Frame::distributeFeatures' grid (Frame.cc:204-210) on the host: grid[c * rows + r] in keypoint order
std::vector<std::vector<int32_t>> host_grid(const dev::GridGeom &G, int32_t n, const float *uv);
// HammingDistance (DescriptorMatching.cc:21-36) over 8 32-bit words
int hamming(const uint8_t *a, const uint8_t *b);

}  // namespace deftri
