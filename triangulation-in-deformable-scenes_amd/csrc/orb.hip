// orb.hip — ORB::describe (reference Modules/Features/ORB.cc:20-90, ORB.h:34-68) restated as it stands, on
// the device and as the sequential host loops a host-only context runs.
//
//   scale tables (ORB.h:39-49)                                  host, float
//   computePyramid (ORB.cc:32-52)                               per level: k_resize (features.hip) of the blurred
//                                                               level above, then k_orb_level: the 19-pixel
//                                                               reflect-101 border of the unblurred level and the
//                                                               7 x 7 integer Gaussian of its interior
//   computeORBDescriptor (:54-90)                               k_orb_describe, one wave per keypoint
//
// OpenCV's parts (the 8-bit bilinear resize, copyMakeBorder, the 8-bit separable Gaussian of this call) are
// restated from their definitions; include/deftri.h states them.  Everything is integer arithmetic but the
// keypoint's centre and the rotated sample offsets, which are float without contraction on both sides; cos
// and sin of the angle come from the host's libm for both context kinds.  The per-pixel and per-sample
// functions are __host__ __device__ and shared by the kernels and the host loops.
//
// One call uploads the image, the keypoints and the resize tables in one copy and downloads descriptors
// and status in one; nothing blocks in between.  The buffers come from the context's arena (OrbState), which
// grows to the largest call and is freed with the context.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "dev_arena.h"
#include "orb.h"

namespace deftri {

namespace dev {

constexpr int kBorder = 19;          // EDGE_THRESHOLD
constexpr int kHalo = 3;             // the 7-tap blur
constexpr int kTileW = 64, kTileH = 32;
constexpr int kPatternLimit = 15;    // the 31-pixel patch

struct BlurKernel { int k[7]; };
struct OrbLevels {
    const uint8_t *img[DEFTRI_FAST_MAX_LEVELS];   // with the border, pitch cols + 38
    int cols[DEFTRI_FAST_MAX_LEVELS], rows[DEFTRI_FAST_MAX_LEVELS];
    float inv[DEFTRI_FAST_MAX_LEVELS];
};
struct OrbKey { float u, v, a, b; int octave; };

// BORDER_REFLECT_101 of index i into [0, n): exact for -n < i < 2 n - 1; the clamp only guards memory for
// the positions of a tile's halo that no output reads
__host__ __device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// the fixed-point column result to 8 bits: s >= 0, and the kernel's sum of 257 needs the saturation
__host__ __device__ __forceinline__ uint8_t blur_finish(int s) {
    const int v = (s + 32768) >> 16;
    return (uint8_t)(v > 255 ? 255 : v);
}

#pragma clang fp contract(off)
// the keypoint's centre in its level, rounded but still float (ORB.cc:27, :58)
__host__ __device__ __forceinline__ void key_centre(const OrbKey &k, float inv, float &cx, float &cy) {
    cx = rintf(k.u * inv);
    cy = rintf(k.v * inv);
}

// pattern point (px, py) of a keypoint with centre (cx, cy): the pixel it reads in the bordered level, or
// false when it lies outside [-19, cols + 19) x [-19, rows + 19), decided before the conversion to int
__host__ __device__ __forceinline__ bool sample_at(float cx, float cy, float a, float b, int px, int py, int cols, int rows,
                                                    int &at) {
    const float fx = (float)px, fy = (float)py;
    const float row = cy + rintf(fx * b + fy * a);
    const float col = cx + rintf(fx * a - fy * b);
    const bool ok = row >= (float)-kBorder && row < (float)(rows + kBorder) && col >= (float)-kBorder && col < (float)(cols + kBorder);
    at = ok ? ((int)row + kBorder) * (cols + 2 * kBorder) + (int)col + kBorder : 0;
    return ok;
}
#pragma clang fp contract(on)

// One level with its border from the unblurred level src [rows x cols, packed]: a workgroup writes 64 x 32
// pixels of dst [(rows + 38) x (cols + 38), packed].  The tile and a 3-pixel halo are staged in LDS with
// reflect-101 indexing, the row pass goes to LDS as int32, the column pass reads it; pixels of the border
// band take the staged (unblurred, reflected) value.  src is read once (plus the halo), dst written once.
__global__ void __launch_bounds__(256)
k_orb_level(const uint8_t *__restrict__ src, int cols, int rows, uint8_t *__restrict__ dst, BlurKernel K) {
    __shared__ uint8_t tile[kTileH + 2 * kHalo][kTileW + 2 * kHalo + 2];
    __shared__ int rowsum[kTileH + 2 * kHalo][kTileW];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bx0 = (int)blockIdx.x * kTileW, by0 = (int)blockIdx.y * kTileH;      // in dst
    const int u0 = bx0 - kBorder - kHalo, v0 = by0 - kBorder - kHalo;              // the staged tile's origin in src
    constexpr int kStageW = kTileW + 2 * kHalo;
    for (int i = tid; i < (kTileH + 2 * kHalo) * kStageW; i += 256) {
        const int y = i / kStageW, x = i - y * kStageW;
        tile[y][x] = src[(size_t)reflect101(v0 + y, rows) * cols + reflect101(u0 + x, cols)];
    }
    __syncthreads();
    for (int y = wave; y < kTileH + 2 * kHalo; y += 4) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) s += K.k[k] * tile[y][lane + k];
        rowsum[y][lane] = s;
    }
    __syncthreads();
    const int W = cols + 2 * kBorder, H = rows + 2 * kBorder;
    const int bx = bx0 + lane, u = bx - kBorder;
    if (bx >= W) return;
    for (int y = wave; y < kTileH; y += 4) {
        const int by = by0 + y, v = by - kBorder;
        if (by >= H) break;
        uint8_t out = tile[y + kHalo][lane + kHalo];
        if (u >= 0 && u < cols && v >= 0 && v < rows) {
            int s = 0;
#pragma unroll
            for (int k = 0; k < 7; k++) s += K.k[k] * rowsum[y + k][lane];
            out = blur_finish(s);
        }
        dst[(size_t)by * W + bx] = out;
    }
}

// One wave per keypoint, the pattern in LDS.  In round r lane l evaluates comparison c = 64 r + l from its
// two samples; the ballot of the results is bytes 8 r .. 8 r + 7 of the descriptor, bit c % 8 of byte c / 8
// being comparison c.  A sample outside the bordered level anywhere in the wave zeroes the descriptor.
__global__ void __launch_bounds__(256)
k_orb_describe(int n, const OrbKey *__restrict__ keys, OrbLevels L, const int8_t *__restrict__ pattern,
               unsigned long long *__restrict__ desc, uint8_t *__restrict__ status) {
    __shared__ int pat[256];                                   // comparison c: x0 y0 x1 y1 as 4 int8
    pat[threadIdx.x] = ((const int *)pattern)[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int k = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (k >= n) return;                                        // the whole wave
    const OrbKey key = keys[k];
    const int level = __builtin_amdgcn_readfirstlane(key.octave);          // the same in every lane
    const int cols = L.cols[level], rows = L.rows[level];
    const uint8_t *img = L.img[level];
    float cx, cy;
    key_centre(key, L.inv[level], cx, cy);
    unsigned long long word[4];
    bool outside = false;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int p = pat[64 * r + lane];
        int at0, at1;
        const bool ok0 = sample_at(cx, cy, key.a, key.b, (int8_t)(p & 255), (int8_t)((p >> 8) & 255), cols, rows, at0);
        const bool ok1 = sample_at(cx, cy, key.a, key.b, (int8_t)((p >> 16) & 255), (int8_t)((p >> 24) & 255), cols, rows, at1);
        outside |= !(ok0 && ok1);
        const int t0 = img[at0], t1 = img[at1];                // at = 0 when outside: a pixel of the level, unused
        word[r] = __ballot(t0 < t1);
    }
    const bool any_outside = __ballot(outside) != 0ull;
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) desc[4 * (size_t)k + r] = any_outside ? 0ull : word[r];
        status[k] = any_outside ? 1 : 0;
    }
}

}  // namespace dev

using namespace dev;

OrbState::~OrbState() {
    if (d_pattern) hipFree(d_pattern);
    if (d_arena) hipFree(d_arena);
    for (hipEvent_t e : ev)
        if (e) hipEventDestroy(e);
}

namespace {

using Clock = std::chrono::steady_clock;
const char *const kEntry = "orb_describe";   // what every argument error of this file starts with

// everything the image size and the parameters decide
struct Plan {
    int n_levels = 0;
    float inv_scale[DEFTRI_FAST_MAX_LEVELS];
    int cols[DEFTRI_FAST_MAX_LEVELS], rows[DEFTRI_FAST_MAX_LEVELS];
    std::vector<Tap> xt[DEFTRI_FAST_MAX_LEVELS], yt[DEFTRI_FAST_MAX_LEVELS];   // level l from level l - 1
    BlurKernel K;
    size_t bordered(int l) const { return (size_t)(rows[l] + 2 * kBorder) * (cols[l] + 2 * kBorder); }
};

int make_plan(const FastImage &im, const deftri_orb_params &p, Plan &P, std::string &err) {
    if (p.n_scales < 1 || p.n_scales > DEFTRI_FAST_MAX_LEVELS) return arg_fail(err, kEntry, "n_scales must be in [1, 16]");
    if (!(p.scale_factor > 1.0f)) return arg_fail(err, kEntry, "scale_factor must be > 1");
    if (im.rows < 1 || im.cols < 1 || im.stride < im.cols) return arg_fail(err, kEntry, "stride < cols, or an empty image");
    const int n = P.n_levels = p.n_scales;
    float scale = 1.0f;                                                    // ORB.h:42-49
    for (int l = 0; l < n; l++) {
        if (l) scale = scale * p.scale_factor;
        P.inv_scale[l] = 1.0f / scale;
        P.cols[l] = cv_round((float)im.cols * P.inv_scale[l]);             // ORB.cc:35
        P.rows[l] = cv_round((float)im.rows * P.inv_scale[l]);
        const std::string at = "level " + std::to_string(l) + " (" + std::to_string(P.cols[l]) + " x " + std::to_string(P.rows[l]) + ")";
        if (P.cols[l] < kBorder + 1 || P.rows[l] < kBorder + 1)
            return arg_fail(err, kEntry, at + " is below the 20 pixels a side the 19-pixel reflected border needs");
        if (l && P.cols[l - 1] == 2 * P.cols[l] && P.rows[l - 1] == 2 * P.rows[l])
            return arg_fail(err, kEntry, at + " halves the level above it exactly: cv::resize takes its area path, which is not restated");
        if (l) {
            P.xt[l] = resize_taps(P.cols[l - 1], P.cols[l]);
            P.yt[l] = resize_taps(P.rows[l - 1], P.rows[l]);
        }
    }
    orb_blur_kernel(P.K.k);
    return 0;
}

// ---- the host loops ------------------------------------------------------------------------------
// one level with its border from the unblurred level src [rows x cols]: copyMakeBorder, then the blur in
// place on the interior, which reads the border just written
void host_level(const uint8_t *src, int cols, int rows, const BlurKernel &K, std::vector<uint8_t> &out) {
    const int W = cols + 2 * kBorder, H = rows + 2 * kBorder;
    out.resize((size_t)W * H);
    for (int by = 0; by < H; by++)
        for (int bx = 0; bx < W; bx++)
            out[(size_t)by * W + bx] = src[(size_t)reflect101(by - kBorder, rows) * cols + reflect101(bx - kBorder, cols)];
    std::vector<int> rowsum((size_t)(rows + 2 * kHalo) * cols);            // rows -3 .. rows + 2 of the interior
    for (int y = 0; y < rows + 2 * kHalo; y++)
        for (int x = 0; x < cols; x++) {
            const uint8_t *p = &out[(size_t)(y + kBorder - kHalo) * W + x + kBorder - kHalo];
            int s = 0;
            for (int k = 0; k < 7; k++) s += K.k[k] * p[k];
            rowsum[(size_t)y * cols + x] = s;
        }
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
            int s = 0;
            for (int k = 0; k < 7; k++) s += K.k[k] * rowsum[(size_t)(y + k) * cols + x];
            out[(size_t)(y + kBorder) * W + x + kBorder] = blur_finish(s);
        }
}

// the interior of a bordered level, packed (the source of the next level's resize)
std::vector<uint8_t> host_interior(const std::vector<uint8_t> &level, int cols, int rows) {
    const int W = cols + 2 * kBorder;
    std::vector<uint8_t> a((size_t)rows * cols);
    for (int y = 0; y < rows; y++) std::memcpy(&a[(size_t)y * cols], &level[(size_t)(y + kBorder) * W + kBorder], (size_t)cols);
    return a;
}

// computeORBDescriptor (:54-90) of one keypoint; true: a sample outside the bordered level, desc zeroed
bool host_describe(const OrbKey &key, const uint8_t *img, int cols, int rows, float inv, const int8_t *pattern, uint8_t *desc) {
    float cx, cy;
    key_centre(key, inv, cx, cy);
    bool outside = false;
    for (int i = 0; i < 32; i++) {
        int val = 0;
        for (int j = 0; j < 8; j++) {
            const int8_t *q = pattern + 4 * (8 * i + j);
            int at0, at1;
            const bool ok0 = sample_at(cx, cy, key.a, key.b, q[0], q[1], cols, rows, at0);
            const bool ok1 = sample_at(cx, cy, key.a, key.b, q[2], q[3], cols, rows, at1);
            outside |= !(ok0 && ok1);
            val |= (img[at0] < img[at1]) << j;
        }
        desc[i] = (uint8_t)val;
    }
    if (outside) std::memset(desc, 0, 32);
    return outside;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// a call's place in the context's arena; the first `upload` bytes mirror the host staging block
struct Layout {
    size_t image = 0, keys = 0, xt[DEFTRI_FAST_MAX_LEVELS] = {}, yt[DEFTRI_FAST_MAX_LEVELS] = {}, upload = 0;
    size_t plain[DEFTRI_FAST_MAX_LEVELS] = {}, level[DEFTRI_FAST_MAX_LEVELS] = {}, out = 0, total = 0;
};

Layout make_layout(const FastImage &im, const Plan &P, size_t n) {
    Layout Y;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
    Y.image = take((size_t)im.rows * im.cols);
    Y.keys = take(sizeof(OrbKey) * n);
    for (int l = 1; l < P.n_levels; l++) { Y.xt[l] = take(sizeof(Tap) * P.xt[l].size()); Y.yt[l] = take(sizeof(Tap) * P.yt[l].size()); }
    Y.upload = at;
    Y.plain[0] = Y.image;                                                 // level 0 unblurred is the image
    for (int l = 1; l < P.n_levels; l++) Y.plain[l] = take((size_t)P.rows[l] * P.cols[l]);
    for (int l = 0; l < P.n_levels; l++) Y.level[l] = take(P.bordered(l));
    Y.out = take(33 * n);                                                 // desc [n * 32], then status [n]
    Y.total = at;
    return Y;
}

int reserve(OrbState &S, size_t bytes, std::string &err) {
    if (bytes > S.arena_size) {
        if (S.d_arena) hipFree(S.d_arena);
        S.d_arena = nullptr;
        S.arena_size = 0;
        const hipError_t e = hipMalloc(&S.d_arena, bytes);
        if (e != hipSuccess) return hip_fail(err, "orb_describe: allocation", e);
        S.arena_size = bytes;
    }
    for (hipEvent_t &e : S.ev)
        if (!e && hipEventCreate(&e) != hipSuccess) { err = "orb_describe: hipEventCreate failed"; return DEFTRI_E_HIP; }
    return 0;
}

// the keypoints as the kernels and the host loops take them: cos and sin by the host's libm (:55-56)
std::vector<OrbKey> make_keys(int32_t n, const float *uv, const int32_t *octave, const float *angle) {
    std::vector<OrbKey> keys((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const float rad = angle[i] * (float)(3.1415926535897932384626433832795 / 180.f);
        keys[i] = {uv[2 * i], uv[2 * i + 1], (float)std::cos((double)rad), (float)std::sin((double)rad), octave[i]};
    }
    return keys;
}

// probe_level >= 0: only the pyramid, that level copied to probe_out
int run(OrbState &S, int device, hipStream_t st, const FastImage &im, const deftri_orb_params &p, int32_t n, const float *uv,
        const int32_t *octave, const float *angle, uint8_t *desc, uint8_t *status, int probe_level, uint8_t *probe_out,
        deftri_orb_report *rep, std::string &err) {
    const auto t_start = Clock::now();
    Plan P;
    if (const int rc = make_plan(im, p, P, err)) return rc;
    const int nl = P.n_levels;
    const bool probe = probe_level >= 0;
    if (probe_level >= nl) return arg_fail(err, kEntry, "level outside [0, n_scales)");
    if (!probe) {
        if (n < 0) return arg_fail(err, kEntry, "n < 0");
        if (!S.have_pattern) return arg_fail(err, kEntry, "no pattern set: pass the 512 sampling points to deftri_orb_set_pattern first");
        for (int32_t i = 0; i < n; i++)
            if (octave[i] < 0 || octave[i] >= nl)
                return arg_fail(err, kEntry, "keypoint " + std::to_string(i) + ": octave " + std::to_string(octave[i]) + " outside [0, n_scales)");
    }
    deftri_orb_report R{};
    R.n_levels = nl;
    R.n_keys = probe ? 0 : n;
    for (int l = 0; l < nl; l++) { R.level_cols[l] = P.cols[l]; R.level_rows[l] = P.rows[l]; }
    if (!probe && n == 0) {
        R.ms_total = ms_since(t_start);
        if (rep) *rep = R;
        return 0;
    }
    const std::vector<OrbKey> keys = probe ? std::vector<OrbKey>() : make_keys(n, uv, octave, angle);
    const size_t nk = keys.size();

    if (device < 0) {
        auto t = Clock::now();
        std::vector<std::vector<uint8_t>> level((size_t)nl);
        std::vector<uint8_t> plain((size_t)im.rows * im.cols);
        for (int y = 0; y < im.rows; y++) std::memcpy(&plain[(size_t)y * im.cols], im.px + (size_t)y * im.stride, (size_t)im.cols);
        for (int l = 0; l < nl; l++) {
            if (l) {
                const std::vector<uint8_t> above = host_interior(level[l - 1], P.cols[l - 1], P.rows[l - 1]);
                plain.resize((size_t)P.rows[l] * P.cols[l]);
                resize_host(above.data(), P.cols[l - 1], plain.data(), P.cols[l], P.rows[l], P.xt[l].data(), P.yt[l].data());
            }
            host_level(plain.data(), P.cols[l], P.rows[l], P.K, level[l]);
        }
        R.ms_pyramid = ms_since(t);
        if (probe) {
            std::memcpy(probe_out, level[probe_level].data(), level[probe_level].size());
            return 0;
        }
        t = Clock::now();
        for (size_t k = 0; k < nk; k++) {
            const int l = keys[k].octave;
            status[k] = host_describe(keys[k], level[l].data(), P.cols[l], P.rows[l], P.inv_scale[l], S.pattern, desc + 32 * k) ? 1 : 0;
            R.n_outside += status[k];
        }
        R.ms_describe = ms_since(t);
        R.ms_total = ms_since(t_start);
        if (rep) *rep = R;
        return 0;
    }

    hipSetDevice(device);
    const Layout Y = make_layout(im, P, nk);
    if (const int rc = reserve(S, Y.total, err)) return rc;
    // the one upload: image, keypoints and resize tables, staged in the arena's order
    std::vector<char> stage(Y.upload);
    for (int y = 0; y < im.rows; y++) std::memcpy(&stage[Y.image + (size_t)y * im.cols], im.px + (size_t)y * im.stride, (size_t)im.cols);
    if (nk) std::memcpy(&stage[Y.keys], keys.data(), sizeof(OrbKey) * nk);
    for (int l = 1; l < nl; l++) {
        std::memcpy(&stage[Y.xt[l]], P.xt[l].data(), sizeof(Tap) * P.xt[l].size());
        std::memcpy(&stage[Y.yt[l]], P.yt[l].data(), sizeof(Tap) * P.yt[l].size());
    }
    char *A = S.d_arena;
    hipMemcpyAsync(A, stage.data(), Y.upload, hipMemcpyHostToDevice, st);
    hipEventRecord(S.ev[0], st);
    OrbLevels L{};
    for (int l = 0; l < nl; l++) {
        uint8_t *plain = (uint8_t *)(A + Y.plain[l]), *level = (uint8_t *)(A + Y.level[l]);
        if (l)   // from the blurred interior of the level above, inside its border
            resize_launch(st, (const uint8_t *)(A + Y.level[l - 1]) + (size_t)kBorder * (P.cols[l - 1] + 2 * kBorder) + kBorder,
                          P.cols[l - 1] + 2 * kBorder, plain, P.cols[l], P.rows[l], (const Tap *)(A + Y.xt[l]), (const Tap *)(A + Y.yt[l]));
        hipLaunchKernelGGL(dev::k_orb_level, dim3((P.cols[l] + 2 * kBorder + kTileW - 1) / kTileW, (P.rows[l] + 2 * kBorder + kTileH - 1) / kTileH),
                           dim3(256), 0, st, plain, P.cols[l], P.rows[l], level, P.K);
        L.img[l] = level; L.cols[l] = P.cols[l]; L.rows[l] = P.rows[l]; L.inv[l] = P.inv_scale[l];
    }
    hipEventRecord(S.ev[1], st);
    if (probe) {
        hipMemcpyAsync(probe_out, A + Y.level[probe_level], P.bordered(probe_level), hipMemcpyDeviceToHost, st);
        const hipError_t e = hipStreamSynchronize(st);
        return e == hipSuccess ? 0 : hip_fail(err, "orb_describe", e);
    }
    hipLaunchKernelGGL(dev::k_orb_describe, dim3((unsigned)((nk + 3) / 4)), dim3(256), 0, st, (int)nk, (const OrbKey *)(A + Y.keys), L,
                       S.d_pattern, (unsigned long long *)(A + Y.out), (uint8_t *)(A + Y.out + 32 * nk));
    hipEventRecord(S.ev[2], st);
    // the one download: descriptors, then status
    std::vector<uint8_t> back(33 * nk);
    hipMemcpyAsync(back.data(), A + Y.out, back.size(), hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(err, "orb_describe", e);
    R.round_trips = 1;
    std::memcpy(desc, back.data(), 32 * nk);
    std::memcpy(status, back.data() + 32 * nk, nk);
    for (size_t k = 0; k < nk; k++) R.n_outside += status[k];
    float ms = 0.0f;
    hipEventElapsedTime(&ms, S.ev[0], S.ev[1]); R.ms_pyramid = ms;
    hipEventElapsedTime(&ms, S.ev[1], S.ev[2]); R.ms_describe = ms;
    R.ms_total = ms_since(t_start);
    if (rep) *rep = R;
    return 0;
}

}  // namespace

// getGaussianKernel(7, 2, CV_32F): exp(-x^2 / (2 sigma^2)) normalized in double and stored as float; the
// 8-bit separable filter takes cvRound(k * 256) of it
void orb_blur_kernel(int32_t *k) {
    const double sigma = 2.0;
    double w[7], sum = 0.0;
    for (int i = 0; i < 7; i++) {
        const double x = i - 3;
        w[i] = std::exp(-(x * x) / (2.0 * sigma * sigma));
        sum += w[i];
    }
    for (int i = 0; i < 7; i++) k[i] = cv_round((float)(w[i] / sum) * 256.0f);
}

int orb_set_pattern(OrbState &S, int device, hipStream_t st, const int32_t *xy, std::string &err) {
    for (int i = 0; i < 1024; i++)
        if (xy[i] < -kPatternLimit || xy[i] > kPatternLimit) {
            err = "orb_set_pattern: point " + std::to_string(i / 2) + (i % 2 ? " y " : " x ") + std::to_string(xy[i]) +
                  " outside [-15, 15], the 31-pixel patch";
            return DEFTRI_E_ARG;
        }
    for (int i = 0; i < 1024; i++) S.pattern[i] = (int8_t)xy[i];
    S.have_pattern = true;
    if (device < 0) return 0;
    hipSetDevice(device);
    hipError_t e = S.d_pattern ? hipSuccess : hipMalloc(&S.d_pattern, sizeof(S.pattern));
    if (e == hipSuccess) e = hipMemcpyAsync(S.d_pattern, S.pattern, sizeof(S.pattern), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        S.have_pattern = false;
        return hip_fail(err, "orb_set_pattern", e);
    }
    return 0;
}

int orb_describe(OrbState &S, int device, hipStream_t st, const FastImage &image, const deftri_orb_params &p, int32_t n,
                 const float *uv, const int32_t *octave, const float *angle, uint8_t *desc, uint8_t *status,
                 deftri_orb_report *report, std::string &err) {
    return run(S, device, st, image, p, n, uv, octave, angle, desc, status, -1, nullptr, report, err);
}

int orb_pyramid_level(OrbState &S, int device, hipStream_t st, const FastImage &image, const deftri_orb_params &p, int32_t level,
                      uint8_t *out, int32_t *out_rows, int32_t *out_cols, std::string &err) {
    if (level < 0) return arg_fail(err, kEntry, "level outside [0, n_scales)");
    Plan P;
    if (const int rc = make_plan(image, p, P, err)) return rc;
    if (level >= P.n_levels) return arg_fail(err, kEntry, "level outside [0, n_scales)");
    *out_rows = P.rows[level] + 2 * kBorder;
    *out_cols = P.cols[level] + 2 * kBorder;
    return run(S, device, st, image, p, 0, nullptr, nullptr, nullptr, nullptr, nullptr, level, out, nullptr, err);
}

}  // namespace deftri
