// features.hip — FAST::extract (reference Modules/Features/FAST.cc:81-118, FAST.h:52-97) restated as it
// stands, on the device and as the sequential host loops a host-only context runs.
//
//   scale tables, features per level (FAST.h:54-78)            host, float
//   computePyramid (:120-139)                                   k_resize, one launch per level
//   cv::FAST per cell, min_th_fast fallback (:168-203)          k_fast_cells, one workgroup per cell
//   distributeOctTree / DivideNode (:243-434, :24-79)           host, sequential, both context kinds
//   GenerateMasks + the mask read (:470-528, :223-234)          k_mask_rows / k_mask_cols: an integral image
//   IC_Angle (:443-467)                                         k_keypoints, one wave per kept keypoint
//
// OpenCV's parts (the 8-bit bilinear resize, FAST-9/16 with non-maximum suppression, fastAtan2) are
// restated from their definitions; include/deftri.h states them.  Everything but the angle is integer
// arithmetic; the angle is float without contraction on both sides.  The per-pixel functions are
// __host__ __device__ and shared by the kernels and the host loops.
//
// The device appends a cell's survivors through one atomic per workgroup, as keys (cell, y, x,
// response); the host sorts them, which is the reference's order (cells row-major, row-major inside a
// cell).  Blocking copy-backs per call: the candidates in front of the octree and the angles and mask
// bits behind it (a third only when there are more than kFirstChunk candidates).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "dev_arena.h"
#include "features.h"

namespace deftri {

namespace dev {

constexpr int kEdge = 16;           // EDGE_THRESHOLD - 3 (:152)
constexpr int kHalfPatch = 15;      // HALF_PATCH_SIZE
constexpr int kTile = 64;           // LDS pitch of a cell's tile; a cell is at most 59 + 6 pixels a side
constexpr int kMaxCellKeys = 1024;  // at most one survivor per 2x2 pixels: 29 * 29 < 1024
constexpr size_t kFirstChunk = 65536;

struct Levels {
    const uint8_t *img[DEFTRI_FAST_MAX_LEVELS];
    int cols[DEFTRI_FAST_MAX_LEVELS], rows[DEFTRI_FAST_MAX_LEVELS];
    int half[DEFTRI_FAST_MAX_LEVELS];   // (side - 1) / 2 of the level's dilation
};
struct CellDesc { int level, x0, y0, w, h, offx, offy, pad; };

// OpenCV's 8-bit bilinear: the horizontal pass in int, the vertical pass with its three shifts
__host__ __device__ __forceinline__ uint8_t resize_pixel(const uint8_t *src, int pitch, const Tap &tx, const Tap &ty) {
    const uint8_t *r0 = src + (size_t)ty.s0 * pitch, *r1 = src + (size_t)ty.s1 * pitch;
    const int h0 = r0[tx.s0] * tx.a0 + r0[tx.s1] * tx.a1;
    const int h1 = r1[tx.s0] * tx.a0 + r1[tx.s1] * tx.a1;
    return (uint8_t)((((ty.a0 * (h0 >> 4)) >> 16) + ((ty.a1 * (h1 >> 4)) >> 16) + 2) >> 2);
}

// cv::FAST's corner score at p (FAST-9/16): s = the maximum over the 16 arcs of 9 contiguous ring pixels
// of the arc's minimum of p_i - c, and of c - p_i; the pixel is a corner at t iff s > t and its response
// is s - 1.  Returns max(s - 1, 0): a corner at t iff the value >= t (t >= 1).
__host__ __device__ __forceinline__ int fast_response(const uint8_t *p, int pitch) {
    const int c = p[0];
    int d[16] = {p[3 * pitch] - c,      p[3 * pitch + 1] - c,  p[2 * pitch + 2] - c,  p[pitch + 3] - c,
                 p[3] - c,              p[-pitch + 3] - c,     p[-2 * pitch + 2] - c, p[-3 * pitch + 1] - c,
                 p[-3 * pitch] - c,     p[-3 * pitch - 1] - c, p[-2 * pitch - 2] - c, p[-pitch - 3] - c,
                 p[-3] - c,             p[pitch - 3] - c,      p[2 * pitch - 2] - c,  p[3 * pitch - 1] - c};
    int lo[16], hi[16], t0[16], t1[16];
    // the minimum and maximum of d[i .. i + 8]: windows of 2, 4, 8, then the ninth
#pragma unroll
    for (int i = 0; i < 16; i++) { lo[i] = min(d[i], d[(i + 1) & 15]); hi[i] = max(d[i], d[(i + 1) & 15]); }
#pragma unroll
    for (int i = 0; i < 16; i++) { t0[i] = min(lo[i], lo[(i + 2) & 15]); t1[i] = max(hi[i], hi[(i + 2) & 15]); }
#pragma unroll
    for (int i = 0; i < 16; i++) { lo[i] = min(t0[i], t0[(i + 4) & 15]); hi[i] = max(t1[i], t1[(i + 4) & 15]); }
    int s = -255;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int mn = min(lo[i], d[(i + 8) & 15]), mx = max(hi[i], d[(i + 8) & 15]);
        s = max(s, max(mn, -mx));
    }
    return s > 1 ? s - 1 : 0;
}

// the response of (x, y) in a cell's map at threshold t: 0 in the cell's 3-pixel margin and below t
__host__ __device__ __forceinline__ int cell_response(const uint8_t *resp, int pitch, int w, int h, int x, int y, int t) {
    if (x < 3 || y < 3 || x >= w - 3 || y >= h - 3) return 0;
    const int r = resp[y * pitch + x];
    return r >= t ? r : 0;
}

// non-maximum suppression: kept iff a corner at t and strictly above its 8 neighbours
__host__ __device__ __forceinline__ bool cell_keeps(const uint8_t *resp, int pitch, int w, int h, int x, int y, int t) {
    const int r = cell_response(resp, pitch, w, h, x, y, t);
    if (r == 0) return false;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++)
            if ((dx || dy) && cell_response(resp, pitch, w, h, x + dx, y + dy, t) >= r) return false;
    return true;
}

// cv::fastAtan2(y, x) in degrees
__host__ __device__ __forceinline__ float fast_atan2_deg(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float eps = (float)2.2204460492503131e-16;
    float a;
    if (ax >= ay) {
        const float c = ay / (ax + eps), c2 = c * c;
        a = (((-2.5397246f * c2 + 8.9140005f) * c2 + -18.667446f) * c2 + 57.283627f) * c;
    } else {
        const float c = ax / (ay + eps), c2 = c * c;
        a = 90.0f - (((-2.5397246f * c2 + 8.9140005f) * c2 + -18.667446f) * c2 + 57.283627f) * c;
    }
    if (x < 0.0f) a = 180.0f - a;
    if (y < 0.0f) a = 360.0f - a;
    return a;
}

// the dilated mask at (x, y): any base-mask pixel in the (2 * half + 1)^2 window clipped to the image.
// S [(rows + 1) * (cols + 1)]: the integral image of the binary base mask.
__host__ __device__ __forceinline__ bool mask_hit(const int32_t *S, int cols, int rows, int x, int y, int half) {
    const int x0 = max(x - half, 0), y0 = max(y - half, 0), x1 = min(x + half, cols - 1) + 1, y1 = min(y + half, rows - 1) + 1;
    if (x0 >= x1 || y0 >= y1) return false;
    const size_t p = (size_t)cols + 1;
    return S[y1 * p + x1] - S[y0 * p + x1] - S[y1 * p + x0] + S[y0 * p + x0] != 0;
}

__host__ __device__ __forceinline__ int base_mask(const uint8_t *img, int pitch, const uint8_t *bm, int bpitch, int x, int y) {
    return (img[(size_t)y * pitch + x] > 240 || (bm && bm[(size_t)y * bpitch + x] != 0)) ? 1 : 0;   // :485-496
}

// one level of the pyramid: 64 x 4 destination pixels per workgroup
__global__ void __launch_bounds__(256) k_resize(const uint8_t *__restrict__ src, int spitch, uint8_t *__restrict__ dst, int dcols,
                                                int drows, const Tap *__restrict__ xt, const Tap *__restrict__ yt) {
    const int x = (int)(blockIdx.x * 64 + (threadIdx.x & 63)), y = (int)(blockIdx.y * 4 + (threadIdx.x >> 6));
    if (x >= dcols || y >= drows) return;
    dst[(size_t)y * dcols + x] = resize_pixel(src, spitch, xt[x], yt[y]);
}

// One workgroup per cell: the tile in LDS, the response of every inner pixel once, the suppression at
// th and, if nothing survives, at min_th.  out[0]: the running number of keys; flags [n cells]: 1 the
// cell fell back, 2 it fell back and stayed empty; keys: (cell << 20) | (y << 14) | (x << 8) | response.
__global__ void __launch_bounds__(256)
k_fast_cells(const CellDesc *__restrict__ cells, Levels L, int th, int min_th, unsigned long long *__restrict__ counter,
             uint8_t *__restrict__ flags, unsigned long long *__restrict__ keys, unsigned long long cap) {
    __shared__ uint8_t tile[kTile * kTile];
    __shared__ uint8_t resp[kTile * kTile];
    __shared__ unsigned int list[kMaxCellKeys];
    __shared__ int cnt;
    __shared__ unsigned long long base;
    const CellDesc c = cells[blockIdx.x];
    const uint8_t *img = L.img[c.level];
    const int pitch = L.cols[c.level];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < c.w * c.h; i += 256) {
        const int y = i / c.w, x = i - y * c.w;
        tile[y * kTile + x] = img[(size_t)(c.y0 + y) * pitch + c.x0 + x];
    }
    if (tid == 0) cnt = 0;
    __syncthreads();
    const int iw = c.w - 6, ih = c.h - 6;
    const int n_in = (iw > 0 && ih > 0) ? iw * ih : 0;
    for (int i = tid; i < n_in; i += 256) {
        const int y = 3 + i / iw, x = 3 + i % iw;
        resp[y * kTile + x] = (uint8_t)fast_response(&tile[y * kTile + x], kTile);
    }
    __syncthreads();
    int flag = 0, found = 0;
    for (int pass = 0; pass < 2; pass++) {
        const int t = pass ? min_th : th;
        for (int i = tid; i < n_in; i += 256) {
            const int y = 3 + i / iw, x = 3 + i % iw;
            if (cell_keeps(resp, kTile, c.w, c.h, x, y, t)) {
                const int slot = atomicAdd(&cnt, 1);
                if (slot < kMaxCellKeys) list[slot] = ((unsigned)y << 14) | ((unsigned)x << 8) | resp[y * kTile + x];
            }
        }
        __syncthreads();
        found = min(cnt, kMaxCellKeys);
        __syncthreads();
        if (found > 0) break;                 // the same for every thread
        flag = pass ? 2 : 1;                  // :189-193
    }
    if (tid == 0) {
        flags[blockIdx.x] = (uint8_t)flag;
        base = found ? atomicAdd(counter, (unsigned long long)found) : 0ull;
    }
    __syncthreads();
    for (int i = tid; i < found; i += 256)
        if (base + i < cap) keys[base + i] = ((unsigned long long)blockIdx.x << 20) | list[i];
}

// the base mask's row sums: one wave per row, R [(rows + 1) * (cols + 1)]
__global__ void __launch_bounds__(256)
k_mask_rows(const uint8_t *__restrict__ img, const uint8_t *__restrict__ bm, int rows, int cols, int32_t *__restrict__ R) {
    const int lane = threadIdx.x & 63;
    const int y = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));   // row y of R, 0 .. rows
    if (y > rows) return;
    int32_t *out = R + (size_t)y * (cols + 1);
    if (lane == 0) out[0] = 0;
    int carry = 0;
    for (int x0 = 0; x0 < cols; x0 += 64) {
        const int x = x0 + lane;
        int v = (y > 0 && x < cols) ? base_mask(img, cols, bm, cols, x, y - 1) : 0;
        for (int off = 1; off < 64; off <<= 1) {
            const int u = __shfl_up(v, off, 64);
            if (lane >= off) v += u;
        }
        if (x < cols) out[x + 1] = carry + v;
        carry += __shfl(v, 63, 64);
    }
}

// the column sums of R: one thread per column
__global__ void k_mask_cols(const int32_t *__restrict__ R, int rows, int cols, int32_t *__restrict__ S) {
    const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (x > cols) return;
    const size_t p = (size_t)cols + 1;
    int acc = 0;
#pragma unroll 8
    for (int y = 0; y <= rows; y++) {
        acc += R[y * p + x];
        S[y * p + x] = acc;
    }
}

// One wave per kept keypoint (level, x, y in level pixels): IC_Angle's moments over the radius-15
// circular patch, two patch rows per step, a butterfly sum, then fastAtan2 and the mask read on lane 0.
__global__ void __launch_bounds__(256)
k_keypoints(int nk, const int *__restrict__ keys, Levels L, const int *__restrict__ umax, const int32_t *__restrict__ S, int cols0,
            int rows0, uint2 *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int k = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (k >= nk) return;
    const int level = keys[3 * k], x = keys[3 * k + 1], y = keys[3 * k + 2];
    const uint8_t *img = L.img[level];
    const int pitch = L.cols[level];
    const int u = (lane & 31) - kHalfPatch;
    int m10 = 0, m01 = 0;
    for (int it = 0; it <= kHalfPatch; it++) {
        const int v = -kHalfPatch + 2 * it + (lane >> 5);
        if (v <= kHalfPatch && u <= kHalfPatch && abs(u) <= umax[abs(v)]) {
            const int val = img[(size_t)(y + v) * pitch + x + u];
            m10 += u * val;
            m01 += v * val;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        m10 += __shfl_xor(m10, off, 64);
        m01 += __shfl_xor(m01, off, 64);
    }
    if (lane == 0) {
        const float a = fast_atan2_deg((float)m01, (float)m10);
        out[k] = make_uint2(__float_as_uint(a), mask_hit(S, cols0, rows0, x, y, L.half[level]) ? 1u : 0u);
    }
}

__global__ void k_mask_reads(int n, const int *__restrict__ xy, const int32_t *__restrict__ S, int cols, int rows, int half,
                             uint8_t *__restrict__ hit) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) hit[i] = mask_hit(S, cols, rows, xy[2 * i], xy[2 * i + 1], half) ? 1 : 0;
}

}  // namespace dev

using namespace dev;

namespace {

using Clock = std::chrono::steady_clock;
const char *const kEntry = "fast_extract";   // what every argument error of this file starts with

struct Cand { int x, y, resp; };       // relative to the 16-pixel border: vToDistributeKeys' pt

// everything the image size and the parameters decide
struct Plan {
    int n_levels = 0;
    float scale[DEFTRI_FAST_MAX_LEVELS], inv_scale[DEFTRI_FAST_MAX_LEVELS];
    int cols[DEFTRI_FAST_MAX_LEVELS], rows[DEFTRI_FAST_MAX_LEVELS], features[DEFTRI_FAST_MAX_LEVELS];
    int half[DEFTRI_FAST_MAX_LEVELS], n_ini[DEFTRI_FAST_MAX_LEVELS];
    std::vector<Tap> xt[DEFTRI_FAST_MAX_LEVELS], yt[DEFTRI_FAST_MAX_LEVELS];   // level l from level l - 1
    std::vector<CellDesc> cells;                                             // every level's, in order
    int cell_begin[DEFTRI_FAST_MAX_LEVELS + 1];
    size_t key_cap[DEFTRI_FAST_MAX_LEVELS];                                    // survivors a level can have
    int umax[kHalfPatch + 1];
};

// OpenCV's tap table of one axis: src -> dst
std::vector<Tap> taps(int src, int dst) {
    std::vector<Tap> t((size_t)dst);
    const double scale = (double)src / dst;
    for (int d = 0; d < dst; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= s;
        int s1 = s + 1;
        if (s < 0) { s = 0; s1 = 1; f = 0.0f; }
        if (s >= src - 1) { s = src - 1; s1 = s; f = 0.0f; }
        t[d] = {s, s1, cv_round((1.0f - f) * 2048.0f), cv_round(f * 2048.0f)};
    }
    return t;
}

// the side of level i's dilation (:510-515)
int mask_side(int level) {
    const float factor = (float)(2.5 / 1.5);
    int max_scale = 1;
    for (int i = 0; i <= level; i++) max_scale *= 2;
    return (int)ceilf(max_scale * factor) * 2 + 5;
}

int make_plan(const FastImage &im, const deftri_fast_params &p, bool with_cells, Plan &P, std::string &err) {
    if (p.n_scales < 1 || p.n_scales > DEFTRI_FAST_MAX_LEVELS) return arg_fail(err, kEntry, "n_scales must be in [1, 16]");
    if (!(p.scale_factor > 1.0f)) return arg_fail(err, kEntry, "scale_factor must be > 1");
    if (im.rows < 1 || im.cols < 1 || im.stride < im.cols) return arg_fail(err, kEntry, "stride < cols, or an empty image");
    if (p.th_fast < 1 || p.th_fast > 255 || p.min_th_fast < 1 || p.min_th_fast > p.th_fast)
        return arg_fail(err, kEntry, "thresholds must satisfy 1 <= min_th_fast <= th_fast <= 255");
    if (p.max_keys < 0) return arg_fail(err, kEntry, "max_keys < 0");
    if (p.n_max_features < 0) return arg_fail(err, kEntry, "n_max_features < 0");
    const int n = P.n_levels = p.n_scales;
    // FAST.h:54-78, in float as written
    P.scale[0] = 1.0f;
    for (int i = 1; i < n; i++) P.scale[i] = P.scale[i - 1] * p.scale_factor;
    for (int i = 0; i < n; i++) P.inv_scale[i] = 1.0f / P.scale[i];
    const float factor = 1.0f / p.scale_factor;
    float desired = (float)p.n_max_features * (1 - factor) / (1 - (float)std::pow((double)factor, (double)n));
    int sum = 0;
    for (int l = 0; l < n - 1; l++) {
        P.features[l] = cv_round(desired);
        sum += P.features[l];
        desired *= factor;
    }
    P.features[n - 1] = std::max(p.n_max_features - sum, 0);
    // umax_ (FAST.h:82-96)
    const int vmax = (int)floorf(kHalfPatch * sqrtf(2.f) / 2 + 1), vmin = (int)ceilf(kHalfPatch * sqrtf(2.f) / 2);
    const double hp2 = kHalfPatch * kHalfPatch;
    for (int v = 0; v <= kHalfPatch; v++) P.umax[v] = 0;
    for (int v = 0; v <= vmax; v++) P.umax[v] = (int)lrint(std::sqrt(hp2 - v * v));
    for (int v = kHalfPatch, v0 = 0; v >= vmin; --v) {
        while (P.umax[v0] == P.umax[v0 + 1]) ++v0;
        P.umax[v] = v0;
        ++v0;
    }
    P.cells.clear();
    for (int l = 0; l < n; l++) {
        P.cols[l] = l ? cv_round((float)im.cols * P.inv_scale[l]) : im.cols;   // :123
        P.rows[l] = l ? cv_round((float)im.rows * P.inv_scale[l]) : im.rows;
        P.half[l] = (mask_side(l) - 1) / 2;
        P.cell_begin[l] = (int)P.cells.size();
        P.key_cap[l] = 0;
        const std::string at = "level " + std::to_string(l) + " (" + std::to_string(P.cols[l]) + " x " + std::to_string(P.rows[l]) + ")";
        if (P.cols[l] < 62 || P.rows[l] < 62)
            return arg_fail(err, kEntry, at + " is below the 62 pixels a side one cell needs (the reference divides by nCols = 0)");
        if (l && P.cols[l - 1] == 2 * P.cols[l] && P.rows[l - 1] == 2 * P.rows[l])
            return arg_fail(err, kEntry, at + " halves the level above it exactly: cv::resize takes its area path, which is not restated");
        if (l) {
            P.xt[l] = taps(P.cols[l - 1], P.cols[l]);
            P.yt[l] = taps(P.rows[l - 1], P.rows[l]);
        }
        // :152-166
        const int min_bx = kEdge, min_by = kEdge, max_bx = P.cols[l] - kEdge, max_by = P.rows[l] - kEdge;
        const float width = (float)(max_bx - min_bx), height = (float)(max_by - min_by);
        const float W = 30;
        const int n_cols = (int)(width / W), n_rows = (int)(height / W);
        const int w_cell = (int)ceilf(width / n_cols), h_cell = (int)ceilf(height / n_rows);
        // distributeOctTree's nIni (:246)
        P.n_ini[l] = (int)roundf((float)(max_bx - min_bx) / (max_by - min_by));
        if (P.n_ini[l] < 1)
            return arg_fail(err, kEntry, at + ": distributeOctTree starts from round(width / height) = 0 nodes and the reference divides by it");
        if (!with_cells) continue;
        for (int i = 0; i < n_rows; i++) {                                 // :168-203
            const float ini_y = (float)(min_by + i * h_cell);
            float max_y = ini_y + h_cell + 6;
            if (ini_y >= max_by - 3) continue;
            if (max_y > max_by) max_y = (float)max_by;
            for (int j = 0; j < n_cols; j++) {
                const float ini_x = (float)(min_bx + j * w_cell);
                float max_x = ini_x + w_cell + 6;
                if (ini_x >= max_bx - 6) continue;
                if (max_x > max_bx) max_x = (float)max_bx;
                CellDesc c{l, (int)ini_x, (int)ini_y, (int)max_x - (int)ini_x, (int)max_y - (int)ini_y, j * w_cell, i * h_cell, 0};
                if (c.w > kTile || c.h > kTile || c.w < 1 || c.h < 1) return arg_fail(err, kEntry, at + ": a cell larger than 64 pixels a side");
                P.cells.push_back(c);
                if (c.w > 6 && c.h > 6) P.key_cap[l] += (size_t)((c.w - 5) / 2) * ((c.h - 5) / 2);
            }
        }
    }
    P.cell_begin[n] = (int)P.cells.size();
    if (P.cells.size() >= ((size_t)1 << 24)) return arg_fail(err, kEntry, "more than 2^24 cells");
    return 0;
}

// ---- distributeOctTree (:243-434) over one level's candidates ----------------------------------
struct Node {
    int x0, y0, x1, y1;                 // UL = (x0, y0), UR.x = x1, BL.y = BR.y = y1
    std::vector<int> keys;
    bool no_more = false;
    int prev = -1, next = -1;
};

struct NodeList {                       // std::list<ExtractorNode>: a node's index is its creation order
    std::vector<Node> pool;
    int head = -1, tail = -1, size = 0;
    int push_back(Node &&n) {
        const int i = (int)pool.size();
        n.prev = tail; n.next = -1;
        pool.push_back(std::move(n));
        if (tail >= 0) pool[tail].next = i; else head = i;
        tail = i; size++;
        return i;
    }
    int push_front(Node &&n) {
        const int i = (int)pool.size();
        n.prev = -1; n.next = head;
        pool.push_back(std::move(n));
        if (head >= 0) pool[head].prev = i; else tail = i;
        head = i; size++;
        return i;
    }
    int erase(int i) {                  // the index after i
        const int p = pool[i].prev, n = pool[i].next;
        if (p >= 0) pool[p].next = n; else head = n;
        if (n >= 0) pool[n].prev = p; else tail = p;
        pool[i].keys = std::vector<int>();
        size--;
        return n;
    }
};

// ExtractorNode::DivideNode (:24-79)
void divide_node(const Node &n, const std::vector<Cand> &cand, Node ch[4]) {
    const int half_x = (int)ceilf((float)(n.x1 - n.x0) / 2), half_y = (int)ceilf((float)(n.y1 - n.y0) / 2);
    const int xm = n.x0 + half_x, ym = n.y0 + half_y;
    ch[0] = Node{n.x0, n.y0, xm, ym};
    ch[1] = Node{xm, n.y0, n.x1, ym};
    ch[2] = Node{n.x0, ym, xm, n.y1};
    ch[3] = Node{xm, ym, n.x1, n.y1};
    for (int k : n.keys) {
        const Cand &c = cand[k];
        if (c.x < xm) ch[c.y < ym ? 0 : 2].keys.push_back(k);
        else ch[c.y < ym ? 1 : 3].keys.push_back(k);
    }
    for (int q = 0; q < 4; q++)
        if (ch[q].keys.size() == 1) ch[q].no_more = true;
}

// the candidates kept, in the order of the reference's result list
std::vector<int> distribute_oct_tree(const std::vector<Cand> &cand, int width, int height, int n_ini, int N) {
    const float hx = (float)width / n_ini;
    NodeList L;
    std::vector<int> ini((size_t)n_ini);
    for (int i = 0; i < n_ini; i++) ini[i] = L.push_back(Node{(int)(hx * (float)i), 0, (int)(hx * (float)(i + 1)), height});
    for (int k = 0; k < (int)cand.size(); k++) {
        const int at = std::min((int)((float)cand[k].x / hx), n_ini - 1);   // :270; the minimum only guards memory
        L.pool[ini[at]].keys.push_back(k);
    }
    for (int it = L.head; it >= 0;) {                                      // :275-284
        if (L.pool[it].keys.size() == 1) { L.pool[it].no_more = true; it = L.pool[it].next; }
        else if (L.pool[it].keys.empty()) it = L.erase(it);
        else it = L.pool[it].next;
    }
    std::vector<std::pair<int, int>> to_expand;                            // (size, node)
    // the children of node `at` to the front of the list, those with more than one key noted; then `at` leaves
    auto split = [&](int at) {
        Node ch[4];
        divide_node(L.pool[at], cand, ch);
        int many = 0;
        for (int q = 0; q < 4; q++) {
            if (ch[q].keys.empty()) continue;
            const int sz = (int)ch[q].keys.size();
            const int id = L.push_front(std::move(ch[q]));
            if (sz > 1) { many++; to_expand.push_back({sz, id}); }
        }
        return many;
    };
    bool finish = false;
    while (!finish) {
        int prev_size = L.size;
        int n_to_expand = 0;
        to_expand.clear();
        for (int it = L.head; it >= 0;) {
            if (L.pool[it].no_more) { it = L.pool[it].next; continue; }
            n_to_expand += split(it);
            it = L.erase(it);
        }
        if (L.size >= N || L.size == prev_size) finish = true;             // :356
        else if (L.size + n_to_expand * 3 > N) {
            while (!finish) {
                prev_size = L.size;
                std::vector<std::pair<int, int>> prev = to_expand;
                to_expand.clear();
                // equal sizes: by creation order, where the reference compares the nodes' addresses
                std::sort(prev.begin(), prev.end());
                for (int j = (int)prev.size() - 1; j >= 0; j--) {
                    split(prev[j].second);
                    L.erase(prev[j].second);
                    if (L.size >= N) break;
                }
                if (L.size >= N || L.size == prev_size) finish = true;
            }
        }
    }
    std::vector<int> kept;
    kept.reserve((size_t)L.size);
    for (int it = L.head; it >= 0; it = L.pool[it].next) {                 // :418-431, the first maximum
        const std::vector<int> &keys = L.pool[it].keys;
        int best = keys[0];
        for (size_t k = 1; k < keys.size(); k++)
            if (cand[keys[k]].resp > cand[best].resp) best = keys[k];
        kept.push_back(best);
    }
    return kept;
}

// ---- the host loops ------------------------------------------------------------------------------
std::vector<uint8_t> host_level0(const FastImage &im) {
    std::vector<uint8_t> a((size_t)im.rows * im.cols);
    for (int y = 0; y < im.rows; y++) std::memcpy(a.data() + (size_t)y * im.cols, im.px + (size_t)y * im.stride, (size_t)im.cols);
    return a;
}

void host_resize(const Plan &P, int l, const std::vector<uint8_t> &src, std::vector<uint8_t> &dst) {
    dst.resize((size_t)P.rows[l] * P.cols[l]);
    for (int y = 0; y < P.rows[l]; y++)
        for (int x = 0; x < P.cols[l]; x++)
            dst[(size_t)y * P.cols[l] + x] = resize_pixel(src.data(), P.cols[l - 1], P.xt[l][x], P.yt[l][y]);
}

// one cell (:185-201): its candidates appended in row-major order; 0, or the cell's flag
int host_cell(const CellDesc &c, const uint8_t *img, int pitch, int th, int min_th, std::vector<Cand> &out) {
    std::vector<uint8_t> resp((size_t)c.w * c.h, 0);
    const uint8_t *tile = img + (size_t)c.y0 * pitch + c.x0;
    for (int y = 3; y < c.h - 3; y++)
        for (int x = 3; x < c.w - 3; x++) resp[(size_t)y * c.w + x] = (uint8_t)fast_response(tile + (size_t)y * pitch + x, pitch);
    for (int pass = 0; pass < 2; pass++) {
        const size_t before = out.size();
        const int t = pass ? min_th : th;
        for (int y = 3; y < c.h - 3; y++)
            for (int x = 3; x < c.w - 3; x++)
                if (cell_keeps(resp.data(), c.w, c.w, c.h, x, y, t)) out.push_back({x + c.offx, y + c.offy, resp[(size_t)y * c.w + x]});
        if (out.size() > before) return pass;
    }
    return 2;
}

std::vector<int32_t> host_integral(const FastImage &im, const FastImage &bm) {
    const size_t p = (size_t)im.cols + 1;
    std::vector<int32_t> S(p * ((size_t)im.rows + 1), 0);
    for (int y = 0; y < im.rows; y++) {
        int run = 0;
        for (int x = 0; x < im.cols; x++) {
            run += base_mask(im.px, im.stride, bm.px, bm.stride, x, y);
            S[(y + 1) * p + x + 1] = S[y * p + x + 1] + run;
        }
    }
    return S;
}

// IC_Angle (:443-467) at (x, y) of a level
float host_angle(const uint8_t *img, int pitch, int x, int y, const int *umax) {
    int m_01 = 0, m_10 = 0;
    const uint8_t *center = img + (size_t)y * pitch + x;
    for (int u = -kHalfPatch; u <= kHalfPatch; ++u) m_10 += u * center[u];
    for (int v = 1; v <= kHalfPatch; ++v) {
        int v_sum = 0;
        const int d = umax[v];
        for (int u = -d; u <= d; ++u) {
            const int val_plus = center[u + v * pitch], val_minus = center[u - v * pitch];
            v_sum += (val_plus - val_minus);
            m_10 += u * (val_plus + val_minus);
        }
        m_01 += v * v_sum;
    }
    return fast_atan2_deg((float)m_01, (float)m_10);
}

bool mask_size_ok(const FastImage &im, const FastImage &bm, std::string &err) {
    if (!bm.px) return true;
    if (bm.rows == im.rows && bm.cols == im.cols && bm.stride >= bm.cols) return true;
    err = "fast_extract: the border mask is " + std::to_string(bm.cols) + " x " + std::to_string(bm.rows) + ", the image " +
          std::to_string(im.cols) + " x " + std::to_string(im.rows) + " (cv::bitwise_or throws)";
    return false;
}

// what a debug entry asks of run()
struct Probe {
    int pyramid_level = -1;
    uint8_t *pyramid_out = nullptr;
    int cand_level = -1;
    std::vector<Cand> *cand_out = nullptr;
};

// the device's buffers of one call
struct DeviceCall {
    DevArena A;
    uint8_t *img[DEFTRI_FAST_MAX_LEVELS] = {};
    uint8_t *bm = nullptr;
    Tap *xt[DEFTRI_FAST_MAX_LEVELS] = {}, *yt[DEFTRI_FAST_MAX_LEVELS] = {};
    CellDesc *cells = nullptr;
    unsigned long long *out = nullptr;   // [0] the number of keys, then the cells' flags, then the keys
    int32_t *R = nullptr, *S = nullptr;
    int *umax = nullptr, *kin = nullptr;
    uint2 *kout = nullptr;
    hipEvent_t ev[4] = {};
    ~DeviceCall() {
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
    }
};

int run(int device, hipStream_t st, const FastImage &im, const FastImage &bm, const deftri_fast_params &p, const Probe &probe,
        float *uv, int32_t *octave, float *angle, float *response, float *size, int32_t *n_keys, deftri_fast_report *rep,
        std::string &err) {
    const auto t_start = Clock::now();
    const bool full = probe.pyramid_level < 0 && probe.cand_level < 0;
    Plan P;
    if (const int rc = make_plan(im, p, probe.pyramid_level < 0, P, err)) return rc;
    if (full && !mask_size_ok(im, bm, err)) return DEFTRI_E_ARG;
    const int nl = P.n_levels;
    if (probe.pyramid_level >= nl || probe.cand_level >= nl) return arg_fail(err, kEntry, "level outside [0, n_scales)");
    deftri_fast_report R{};
    R.n_levels = nl;
    for (int l = 0; l < nl; l++) { R.level_cols[l] = P.cols[l]; R.level_rows[l] = P.rows[l]; R.features_per_level[l] = P.features[l]; }
    const int ncell = (int)P.cells.size();
    std::vector<std::vector<Cand>> cand((size_t)nl);
    std::vector<uint8_t> flags((size_t)ncell, 0);
    std::vector<std::vector<uint8_t>> pyr;          // host-only
    DeviceCall D;                                   // device
    size_t key_cap = 0, kept_cap = 0;
    for (int l = 0; l < nl; l++) {
        key_cap += P.key_cap[l];
        kept_cap += std::min(P.key_cap[l], (size_t)4 * std::max(P.features[l], P.n_ini[l]));
    }
    const size_t flag_words = ((size_t)ncell + 7) / 8;

    // ---- pyramid and cells ----
    if (device < 0) {
        auto t = Clock::now();
        pyr.resize((size_t)nl);
        pyr[0] = host_level0(im);
        for (int l = 1; l < nl; l++) host_resize(P, l, pyr[l - 1], pyr[l]);
        R.ms_resize = ms_since(t);
        if (probe.pyramid_level >= 0) {
            std::memcpy(probe.pyramid_out, pyr[probe.pyramid_level].data(), pyr[probe.pyramid_level].size());
            return 0;
        }
        t = Clock::now();
        for (int l = 0; l < nl; l++)
            for (int c = P.cell_begin[l]; c < P.cell_begin[l + 1]; c++)
                flags[c] = (uint8_t)host_cell(P.cells[c], pyr[l].data(), P.cols[l], p.th_fast, p.min_th_fast, cand[l]);
        R.ms_cells = ms_since(t);
    } else {
        hipSetDevice(device);
        for (int l = 0; l < nl; l++) {
            D.A.add(&D.img[l], (size_t)P.rows[l] * P.cols[l]);
            if (l) { D.A.add(&D.xt[l], P.xt[l].size()); D.A.add(&D.yt[l], P.yt[l].size()); }
        }
        if (full) {
            if (bm.px) D.A.add(&D.bm, (size_t)im.rows * im.cols);
            D.A.add(&D.R, ((size_t)im.rows + 1) * ((size_t)im.cols + 1));
            D.A.add(&D.S, ((size_t)im.rows + 1) * ((size_t)im.cols + 1));
            D.A.add(&D.umax, kHalfPatch + 1);
            D.A.add(&D.kin, 3 * kept_cap);
            D.A.add(&D.kout, kept_cap);
        }
        D.A.add(&D.cells, (size_t)ncell);
        D.A.add(&D.out, 1 + flag_words + key_cap);
        if (!D.A.commit()) {
            err = "fast_extract: allocation failed";
            return DEFTRI_E_HIP;
        }
        for (hipEvent_t &e : D.ev)
            if (hipEventCreate(&e) != hipSuccess) { err = "fast_extract: hipEventCreate failed"; return DEFTRI_E_HIP; }
        Levels L{};
        for (int l = 0; l < nl; l++) { L.img[l] = D.img[l]; L.cols[l] = P.cols[l]; L.rows[l] = P.rows[l]; L.half[l] = P.half[l]; }
        hipEventRecord(D.ev[0], st);
        hipMemcpy2DAsync(D.img[0], (size_t)im.cols, im.px, (size_t)im.stride, (size_t)im.cols, (size_t)im.rows, hipMemcpyHostToDevice, st);
        for (int l = 1; l < nl; l++) {
            hipMemcpyAsync(D.xt[l], P.xt[l].data(), sizeof(Tap) * P.xt[l].size(), hipMemcpyHostToDevice, st);
            hipMemcpyAsync(D.yt[l], P.yt[l].data(), sizeof(Tap) * P.yt[l].size(), hipMemcpyHostToDevice, st);
            hipLaunchKernelGGL(dev::k_resize, dim3((P.cols[l] + 63) / 64, (P.rows[l] + 3) / 4), dim3(256), 0, st, D.img[l - 1],
                               P.cols[l - 1], D.img[l], P.cols[l], P.rows[l], D.xt[l], D.yt[l]);
        }
        hipEventRecord(D.ev[1], st);
        if (probe.pyramid_level >= 0) {
            const int l = probe.pyramid_level;
            hipMemcpyAsync(probe.pyramid_out, D.img[l], (size_t)P.rows[l] * P.cols[l], hipMemcpyDeviceToHost, st);
            const hipError_t e = hipStreamSynchronize(st);
            return e == hipSuccess ? 0 : hip_fail(err, "fast_extract", e);
        }
        unsigned long long *d_keys = D.out + 1 + flag_words;
        hipMemsetAsync(D.out, 0, sizeof(unsigned long long), st);
        if (ncell) {
            hipMemcpyAsync(D.cells, P.cells.data(), sizeof(CellDesc) * (size_t)ncell, hipMemcpyHostToDevice, st);
            hipLaunchKernelGGL(dev::k_fast_cells, dim3((unsigned)ncell), dim3(256), 0, st, D.cells, L, p.th_fast, p.min_th_fast, D.out,
                               (uint8_t *)(D.out + 1), d_keys, (unsigned long long)key_cap);
        }
        hipEventRecord(D.ev[2], st);
        // the header and the first keys in one copy; the rest, if any, in a second
        const size_t first = std::min(key_cap, kFirstChunk);
        std::vector<unsigned long long> back(1 + flag_words + first);
        hipMemcpyAsync(back.data(), D.out, sizeof(unsigned long long) * (1 + flag_words + first), hipMemcpyDeviceToHost, st);
        hipEventRecord(D.ev[3], st);
        if (full) {
            // the base mask's integral image runs under the host's octree
            if (bm.px)
                hipMemcpy2DAsync(D.bm, (size_t)im.cols, bm.px, (size_t)bm.stride, (size_t)im.cols, (size_t)im.rows, hipMemcpyHostToDevice, st);
            hipMemcpyAsync(D.umax, P.umax, sizeof(P.umax), hipMemcpyHostToDevice, st);
            hipLaunchKernelGGL(dev::k_mask_rows, dim3((im.rows + 1 + 3) / 4), dim3(256), 0, st, D.img[0], D.bm, im.rows, im.cols, D.R);
            hipLaunchKernelGGL(dev::k_mask_cols, dim3((im.cols + 1 + 255) / 256), dim3(256), 0, st, D.R, im.rows, im.cols, D.S);
        }
        hipError_t e = hipEventSynchronize(D.ev[3]);
        if (e != hipSuccess) return hip_fail(err, "fast_extract", e);
        R.round_trips++;
        const size_t nkeys = (size_t)back[0];
        if (nkeys > key_cap) { err = "fast_extract: more candidates than a cell grid can hold"; return DEFTRI_E_NUMERIC; }
        if (nkeys > first) {
            back.resize(1 + flag_words + nkeys);
            e = hipMemcpy(back.data() + 1 + flag_words + first, d_keys + first, sizeof(unsigned long long) * (nkeys - first),
                          hipMemcpyDeviceToHost);
            if (e != hipSuccess) return hip_fail(err, "fast_extract", e);
            R.round_trips++;
        }
        float ms = 0.0f;
        hipEventElapsedTime(&ms, D.ev[0], D.ev[1]); R.ms_resize = ms;
        hipEventElapsedTime(&ms, D.ev[1], D.ev[2]); R.ms_cells = ms;
        std::memcpy(flags.data(), back.data() + 1, (size_t)ncell);
        // (cell, y, x) is the reference's order: the keys to their cells by counting, then each cell's few keys sorted
        const unsigned long long *keys = back.data() + 1 + flag_words;
        std::vector<uint32_t> start((size_t)ncell + 1, 0), in_cell(nkeys);
        for (size_t k = 0; k < nkeys; k++) {
            const size_t c = (size_t)(keys[k] >> 20);
            if (c >= (size_t)ncell) { err = "fast_extract: a key of no cell"; return DEFTRI_E_NUMERIC; }
            start[c + 1]++;
        }
        for (int c = 0; c < ncell; c++) start[c + 1] += start[c];
        std::vector<uint32_t> cursor(start.begin(), start.end() - 1);
        for (size_t k = 0; k < nkeys; k++) in_cell[cursor[keys[k] >> 20]++] = (uint32_t)(keys[k] & 0xfffff);
        for (int l = 0; l < nl; l++) cand[l].reserve(start[P.cell_begin[l + 1]] - start[P.cell_begin[l]]);
        for (int c = 0; c < ncell; c++) {
            std::sort(in_cell.begin() + start[c], in_cell.begin() + start[c + 1]);
            const CellDesc &cd = P.cells[c];
            for (uint32_t k = start[c]; k < start[c + 1]; k++)
                cand[cd.level].push_back({(int)((in_cell[k] >> 8) & 63) + cd.offx, (int)((in_cell[k] >> 14) & 63) + cd.offy, (int)(in_cell[k] & 255)});
        }
    }
    for (int l = 0; l < nl; l++) {
        R.n_candidates[l] = (int32_t)cand[l].size();
        for (int c = P.cell_begin[l]; c < P.cell_begin[l + 1]; c++) {
            if (flags[c]) R.n_fallback_cells[l]++;
            if (flags[c] == 2) R.n_empty_cells[l]++;
        }
    }
    if (probe.cand_level >= 0) {
        *probe.cand_out = std::move(cand[probe.cand_level]);
        return 0;
    }

    // ---- the octree, on the host ----
    auto t = Clock::now();
    std::vector<int> k_level, k_x, k_y, k_resp;      // the kept keypoints of every level, level pixels
    for (int l = 0; l < nl; l++) {
        const std::vector<int> kept = distribute_oct_tree(cand[l], P.cols[l] - 2 * kEdge, P.rows[l] - 2 * kEdge, P.n_ini[l], P.features[l]);
        R.n_octree[l] = (int32_t)kept.size();
        for (int k : kept) {
            k_level.push_back(l);
            k_x.push_back(cand[l][k].x + kEdge);                            // :217-218
            k_y.push_back(cand[l][k].y + kEdge);
            k_resp.push_back(cand[l][k].resp);
        }
    }
    R.ms_octree = ms_since(t);

    // ---- the mask and the orientation of the kept keypoints ----
    t = Clock::now();
    const size_t nk = k_level.size();
    std::vector<float> k_angle(nk);
    std::vector<uint8_t> k_masked(nk);
    if (device < 0) {
        const std::vector<int32_t> S = host_integral(im, bm);
        for (size_t k = 0; k < nk; k++) {
            const int l = k_level[k];
            k_masked[k] = mask_hit(S.data(), im.cols, im.rows, k_x[k], k_y[k], P.half[l]) ? 1 : 0;
            k_angle[k] = host_angle(pyr[l].data(), P.cols[l], k_x[k], k_y[k], P.umax);
        }
    } else if (nk) {
        if (nk > kept_cap) { err = "fast_extract: more kept keypoints than the octree's bound"; return DEFTRI_E_NUMERIC; }
        std::vector<int> kin(3 * nk);
        for (size_t k = 0; k < nk; k++) { kin[3 * k] = k_level[k]; kin[3 * k + 1] = k_x[k]; kin[3 * k + 2] = k_y[k]; }
        std::vector<uint2> kout(nk);
        Levels L{};
        for (int l = 0; l < nl; l++) { L.img[l] = D.img[l]; L.cols[l] = P.cols[l]; L.rows[l] = P.rows[l]; L.half[l] = P.half[l]; }
        hipMemcpyAsync(D.kin, kin.data(), sizeof(int) * 3 * nk, hipMemcpyHostToDevice, st);
        hipLaunchKernelGGL(dev::k_keypoints, dim3((unsigned)((nk + 3) / 4)), dim3(256), 0, st, (int)nk, D.kin, L, D.umax, D.S, im.cols,
                           im.rows, D.kout);
        hipMemcpyAsync(kout.data(), D.kout, sizeof(uint2) * nk, hipMemcpyDeviceToHost, st);
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(err, "fast_extract", e);
        R.round_trips++;
        for (size_t k = 0; k < nk; k++) {
            std::memcpy(&k_angle[k], &kout[k].x, sizeof(float));
            k_masked[k] = (uint8_t)kout[k].y;
        }
    } else {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(err, "fast_extract", e);
    }

    // ---- :98-117 ----
    int32_t n_out = 0;
    for (size_t k = 0; k < nk; k++) {
        const int l = k_level[k];
        if (k_masked[k]) continue;                                           // :223-234
        R.n_after_mask[l]++;
        if (n_out >= p.max_keys) { R.n_truncated[l]++; continue; }          // :110
        uv[2 * n_out] = (float)k_x[k] * P.scale[l];                          // :111
        uv[2 * n_out + 1] = (float)k_y[k] * P.scale[l];
        octave[n_out] = l;
        angle[n_out] = k_angle[k];
        response[n_out] = (float)k_resp[k];
        size[n_out] = (float)(int)(31 * P.scale[l]);                         // :211
        n_out++;
    }
    R.ms_keypoints = ms_since(t);
    R.n_keys = n_out;
    *n_keys = n_out;
    R.ms_total = ms_since(t_start);
    if (rep) *rep = R;
    return 0;
}

}  // namespace

// ---- the 8-bit bilinear resize, shared with ORB::describe's pyramid (orb.hip) ----
std::vector<dev::Tap> resize_taps(int src, int dst) { return taps(src, dst); }

void resize_launch(hipStream_t st, const uint8_t *src, int spitch, uint8_t *dst, int dcols, int drows, const dev::Tap *xt,
                   const dev::Tap *yt) {
    hipLaunchKernelGGL(dev::k_resize, dim3((dcols + 63) / 64, (drows + 3) / 4), dim3(256), 0, st, src, spitch, dst, dcols, drows, xt, yt);
}

void resize_host(const uint8_t *src, int spitch, uint8_t *dst, int dcols, int drows, const dev::Tap *xt, const dev::Tap *yt) {
    for (int y = 0; y < drows; y++)
        for (int x = 0; x < dcols; x++) dst[(size_t)y * dcols + x] = resize_pixel(src, spitch, xt[x], yt[y]);
}

int fast_extract(int device, hipStream_t st, const FastImage &image, const FastImage &border_mask, const deftri_fast_params &p,
                 float *uv, int32_t *octave, float *angle, float *response, float *size, int32_t *n_keys,
                 deftri_fast_report *report, std::string &err) {
    return run(device, st, image, border_mask, p, Probe{}, uv, octave, angle, response, size, n_keys, report, err);
}

int fast_pyramid_level(int device, hipStream_t st, const FastImage &image, const deftri_fast_params &p, int32_t level, uint8_t *out,
                       int32_t *out_rows, int32_t *out_cols, std::string &err) {
    if (level < 0) return arg_fail(err, kEntry, "level outside [0, n_scales)");
    Plan P;
    if (const int rc = make_plan(image, p, false, P, err)) return rc;
    if (level >= P.n_levels) return arg_fail(err, kEntry, "level outside [0, n_scales)");
    *out_rows = P.rows[level];
    *out_cols = P.cols[level];
    Probe probe;
    probe.pyramid_level = level;
    probe.pyramid_out = out;
    return run(device, st, image, FastImage{nullptr, 0, 0, 0}, p, probe, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, err);
}

int fast_candidates(int device, hipStream_t st, const FastImage &image, const deftri_fast_params &p, int32_t level, int32_t max_cand,
                    int32_t *xy, float *response, int32_t *n, std::string &err) {
    if (level < 0) return arg_fail(err, kEntry, "level outside [0, n_scales)");
    std::vector<Cand> cand;
    Probe probe;
    probe.cand_level = level;
    probe.cand_out = &cand;
    if (const int rc = run(device, st, image, FastImage{nullptr, 0, 0, 0}, p, probe, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, err))
        return rc;
    *n = (int32_t)cand.size();
    for (int32_t k = 0; k < *n && k < max_cand; k++) {
        xy[2 * k] = cand[k].x;
        xy[2 * k + 1] = cand[k].y;
        response[k] = (float)cand[k].resp;
    }
    return 0;
}

int fast_mask_reads(int device, hipStream_t st, const FastImage &image, const FastImage &border_mask, int32_t level, int32_t n,
                    const int32_t *xy, uint8_t *hit, std::string &err) {
    if (level < 0 || level >= DEFTRI_FAST_MAX_LEVELS) return arg_fail(err, kEntry, "level outside [0, 16)");
    if (image.rows < 1 || image.cols < 1 || image.stride < image.cols) return arg_fail(err, kEntry, "stride < cols, or an empty image");
    if (!mask_size_ok(image, border_mask, err)) return DEFTRI_E_ARG;
    for (int32_t i = 0; i < n; i++)
        if (xy[2 * i] < 0 || xy[2 * i] >= image.cols || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= image.rows)
            return arg_fail(err, kEntry, "a mask read outside the image");
    const int half = (mask_side(level) - 1) / 2;
    if (device < 0 || n == 0) {
        const std::vector<int32_t> S = host_integral(image, border_mask);
        for (int32_t i = 0; i < n; i++) hit[i] = mask_hit(S.data(), image.cols, image.rows, xy[2 * i], xy[2 * i + 1], half) ? 1 : 0;
        return 0;
    }
    hipSetDevice(device);
    const size_t px = (size_t)image.rows * image.cols, sz = ((size_t)image.rows + 1) * ((size_t)image.cols + 1);
    DevArena A;
    uint8_t *d_img, *d_bm = nullptr, *d_hit;
    int32_t *d_R, *d_S;
    int *d_xy;
    A.add(&d_img, px);
    if (border_mask.px) A.add(&d_bm, px);
    A.add(&d_R, sz); A.add(&d_S, sz); A.add(&d_xy, 2 * (size_t)n); A.add(&d_hit, (size_t)n);
    if (!A.commit()) {
        err = "fast_extract: allocation failed";
        return DEFTRI_E_HIP;
    }
    hipMemcpy2DAsync(d_img, (size_t)image.cols, image.px, (size_t)image.stride, (size_t)image.cols, (size_t)image.rows, hipMemcpyHostToDevice,
                     st);
    if (border_mask.px)
        hipMemcpy2DAsync(d_bm, (size_t)image.cols, border_mask.px, (size_t)border_mask.stride, (size_t)image.cols, (size_t)image.rows,
                         hipMemcpyHostToDevice, st);
    hipMemcpyAsync(d_xy, xy, sizeof(int) * 2 * (size_t)n, hipMemcpyHostToDevice, st);
    hipLaunchKernelGGL(dev::k_mask_rows, dim3((image.rows + 1 + 3) / 4), dim3(256), 0, st, d_img, d_bm, image.rows, image.cols, d_R);
    hipLaunchKernelGGL(dev::k_mask_cols, dim3((image.cols + 1 + 255) / 256), dim3(256), 0, st, d_R, image.rows, image.cols, d_S);
    hipLaunchKernelGGL(dev::k_mask_reads, dim3((n + 255) / 256), dim3(256), 0, st, n, d_xy, d_S, image.cols, image.rows, half, d_hit);
    hipMemcpyAsync(hit, d_hit, (size_t)n, hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : hip_fail(err, "fast_extract", e);
}

}  // namespace deftri
