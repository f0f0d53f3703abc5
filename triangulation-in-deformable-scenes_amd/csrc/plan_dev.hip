// plan_dev.hip — the one-pair tile plan's sorts, scans and numberings on the device (plan_dev.h).
//
// No workgroup waits on another: a scan over more than one workgroup's elements is three launches (tile sums,
// the scan of the sums by one workgroup, the tiles' own scans), a sort by a dense key (a row, a group) is count,
// scan, fill through an atomic cursor and then every key's run put in ascending order, so the result does not
// depend on the order the atomics finished in.  The 42-bit curve key is sorted by a stable LSD radix sort of
// 7-bit digits: per-tile digit counts, one scan of the (digit, tile) table, and a stable rank inside the tile.
// Every loop is bounded; one that reaches its bound sets a word the host reads with the stage's download.
#include "plan_dev.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "spcg.h"

namespace deftri {

namespace {

constexpr int kBlk = 256;                 // threads per workgroup of the element-wise kernels
constexpr int kGridMax = 1 << 16;         // workgroups per launch at most; the rest is strided
constexpr int kRadixDigits = 1 << kPlanRadixBits;
constexpr int kRadixPasses = 42 / kPlanRadixBits;
static_assert(kRadixPasses * kPlanRadixBits == 42, "the passes cover the curve key exactly");
static_assert(kPlanScanTile == 8 * kBlk && kPlanRadixTile == kBlk, "one workgroup per tile");
enum { kHdrBound = 0, kHdrNg = 1, kHdrNrot = 2, kHdrWords = 16 };

namespace dev {

#define PLAN_FOR(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// ---- scans -----------------------------------------------------------------------------------------
// exclusive prefix of v over the workgroup (s: blockDim.x ints of LDS), *total the workgroup's sum
__device__ inline int block_excl_scan(int v, int *s, int *total) {
    const int t = threadIdx.x, n = blockDim.x;
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < n; o <<= 1) {
        const int a = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += a;
        __syncthreads();
    }
    const int inc = s[t];
    *total = s[n - 1];
    __syncthreads();
    return inc - v;
}

__global__ __launch_bounds__(kBlk) void k_scan_reduce(int64_t n, const int *in, int *part, int ntile) {
    __shared__ int s[kBlk];
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t base = (int64_t)tile * kPlanScanTile + 8 * threadIdx.x;
        int sum = 0;
        for (int j = 0; j < 8; j++) if (base + j < n) sum += in[base + j];
        int tot;
        block_excl_scan(sum, s, &tot);
        if (threadIdx.x == 0) part[tile] = tot;
    }
}

__global__ __launch_bounds__(1024) void k_scan_part(int ntile, int *part) {
    __shared__ int s[1024];
    int carry = 0;
    for (int base = 0; base < ntile; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < ntile ? part[i] : 0;
        int tot;
        const int ex = block_excl_scan(v, s, &tot);
        if (i < ntile) part[i] = carry + ex;
        carry += tot;
    }
}

// in place: a thread reads its 8 elements before it writes them, and no other thread touches them
__global__ __launch_bounds__(kBlk) void k_scan_apply(int64_t n, int *data, const int *part, int ntile) {
    __shared__ int s[kBlk];
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t base = (int64_t)tile * kPlanScanTile + 8 * threadIdx.x;
        int v[8], sum = 0;
        for (int j = 0; j < 8; j++) { v[j] = base + j < n ? data[base + j] : 0; sum += v[j]; }
        int tot;
        int run = block_excl_scan(sum, s, &tot) + (part ? part[tile] : 0);
        for (int j = 0; j < 8; j++)
            if (base + j < n) { data[base + j] = run; run += v[j]; }
    }
}

// ---- stage 1: groups -------------------------------------------------------------------------------
__device__ inline int ld_par(const int *par, int a) { return __hip_atomic_load(par + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of a's tree; a parent is always smaller than its child, so the walk ends within P steps (-1: it did not)
__device__ inline int uf_find(int *par, int a, int P, bool halve) {
    for (int step = 0; step <= P; step++) {
        const int p = ld_par(par, a);
        if (p == a) return a;
        if (halve) {
            const int gp = ld_par(par, p);
            if (gp != p) atomicCAS(par + a, p, gp);
        }
        a = p;
    }
    return -1;
}

// spcg_plan.cpp's unite: a root is only ever linked under a smaller root.  A failed compare-and-swap means
// another thread linked that root, which is progress; no thread waits for a particular other thread
__device__ inline bool uf_unite(int *par, int a, int b, int P) {
    for (int t = 0; t < kPlanHookRetries; t++) {
        a = uf_find(par, a, P, true);
        b = uf_find(par, b, P, true);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        if (a > b) { const int c = a; a = b; b = c; }
        if (atomicCAS(par + b, b, a) == b) return true;
    }
    return false;
}

__global__ __launch_bounds__(kBlk) void k_iota(int64_t n, int *a) {
    PLAN_FOR(i, n) a[i] = (int)i;
}

__global__ __launch_bounds__(kBlk) void k_fill(int64_t n, int *a, int v) {
    PLAN_FOR(i, n) a[i] = v;
}

__global__ __launch_bounds__(kBlk) void k_uf_hook(int64_t E, const int4 *ap, int *par, int P, int *hdr) {
    PLAN_FOR(e, E) {
        const int4 v = ap[e];
        const bool a = uf_unite(par, v.x, v.y, P), b = uf_unite(par, v.z, v.w, P);
        if (!a || !b) hdr[kHdrBound] = 1;
    }
}

// after the hooking launch has finished: every point's root, and the roots flagged
__global__ __launch_bounds__(kBlk) void k_uf_flatten(int P, int *par, int *root, int *flag, int *hdr) {
    PLAN_FOR(p, P) {
        int r = uf_find(par, (int)p, P, false);
        if (r < 0) { hdr[kHdrBound] = 1; r = (int)p; }
        root[p] = r;
        flag[p] = r == (int)p;
    }
}

// rank: the exclusive scan of the root flags (P + 1 entries), so rank[root] numbers the roots in ascending id order
__global__ __launch_bounds__(kBlk) void k_groups(int P, const int *root, const int *rank, int *gid, int *grep, int *hdr) {
    PLAN_FOR(p, P) {
        const int r = root[p];
        gid[p] = rank[r];
        if (r == (int)p) grep[rank[p]] = (int)p;
        if (p == 0) hdr[kHdrNg] = rank[P];
    }
}

// ---- stage 2: Morton order -------------------------------------------------------------------------
__device__ inline void minmax_reduce(double v[4], double *s) {      // s: 4 * blockDim.x doubles; result in thread 0's v
    const int t = threadIdx.x;
    for (int c = 0; c < 4; c++) s[c * blockDim.x + t] = v[c];
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if (t < o)
            for (int c = 0; c < 4; c++) {
                const double a = s[c * blockDim.x + t], b = s[c * blockDim.x + t + o];
                s[c * blockDim.x + t] = c < 2 ? (b < a ? b : a) : (b > a ? b : a);
            }
        __syncthreads();
    }
    for (int c = 0; c < 4; c++) v[c] = s[c * blockDim.x];
    __syncthreads();
}

// v: lo x, lo y, hi x, hi y over the finite coordinates of the representatives
__global__ __launch_bounds__(kBlk) void k_minmax_part(const int *ngp, const int *grep, const double *xy, int stride, double *part) {
    __shared__ double s[4 * kBlk];
    const int ng = *ngp;
    double v[4] = {1e300, 1e300, -1e300, -1e300};
    PLAN_FOR(g, ng) {
        const double *q = xy + (int64_t)stride * grep[g];
        for (int c = 0; c < 2; c++) {
            const double x = q[c];
            if (isfinite(x)) { v[c] = x < v[c] ? x : v[c]; v[2 + c] = x > v[2 + c] ? x : v[2 + c]; }
        }
    }
    minmax_reduce(v, s);
    if (threadIdx.x == 0)
        for (int c = 0; c < 4; c++) part[4 * blockIdx.x + c] = v[c];
}

__global__ __launch_bounds__(kBlk) void k_minmax_final(int nparts, const double *part, double *lohi) {
    __shared__ double s[4 * kBlk];
    double v[4] = {1e300, 1e300, -1e300, -1e300};
    for (int i = threadIdx.x; i < nparts; i += blockDim.x)
        for (int c = 0; c < 4; c++) {
            const double x = part[4 * i + c];
            v[c] = c < 2 ? (x < v[c] ? x : v[c]) : (x > v[c] ? x : v[c]);
        }
    minmax_reduce(v, s);
    if (threadIdx.x == 0)
        for (int c = 0; c < 4; c++) lohi[c] = v[c];
}

__global__ __launch_bounds__(kBlk) void k_keys(const int *ngp, const int *grep, const double *xy, int stride, const double *lohi,
                                              uint64_t *key, int *id) {
    const int ng = *ngp;
    const double lo[2] = {lohi[0], lohi[1]}, hi[2] = {lohi[2], lohi[3]};
    PLAN_FOR(g, ng) {
        const double *q = xy + (int64_t)stride * grep[g];
        key[g] = curve_key(q[0], q[1], lo, hi);
        id[g] = (int)g;
    }
}

// one pass of the radix sort: hist[digit][tile] (every tile of the launch writes its column, zeros past ng)
__global__ __launch_bounds__(kBlk) void k_radix_hist(const int *ngp, const uint64_t *key, int shift, int *hist, int ntile) {
    __shared__ int h[kRadixDigits];
    const int ng = *ngp;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        if (threadIdx.x < kRadixDigits) h[threadIdx.x] = 0;
        __syncthreads();
        const int64_t i = (int64_t)tile * kPlanRadixTile + threadIdx.x;
        if (i < ng) atomicAdd(&h[(int)(key[i] >> shift) & (kRadixDigits - 1)], 1);
        __syncthreads();
        if (threadIdx.x < kRadixDigits) hist[(int64_t)threadIdx.x * ntile + tile] = h[threadIdx.x];
        __syncthreads();
    }
}

// base: the exclusive scan of hist.  An item's place is its (digit, tile) base plus the number of earlier items
// of its tile with its digit: stable
__global__ __launch_bounds__(kBlk) void k_radix_scatter(const int *ngp, const uint64_t *key_in, const int *id_in, int shift,
                                                       const int *base, int ntile, uint64_t *key_out, int *id_out) {
    __shared__ unsigned short sd[kPlanRadixTile];
    const int ng = *ngp;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        if ((int64_t)tile * kPlanRadixTile >= ng) break;
        const int t = threadIdx.x;
        const int64_t i = (int64_t)tile * kPlanRadixTile + t;
        uint64_t k = 0;
        int d = 0xffff;
        if (i < ng) { k = key_in[i]; d = (int)(k >> shift) & (kRadixDigits - 1); }
        sd[t] = (unsigned short)d;
        __syncthreads();
        if (i < ng) {
            int r = 0;
            for (int j = 0; j < t; j++) r += sd[j] == d;
            const int pos = base[(int64_t)d * ntile + tile] + r;
            key_out[pos] = k;
            id_out[pos] = id_in[i];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlk) void k_gpos(const int *ngp, const int *gorder, int *gpos) {
    const int ng = *ngp;
    PLAN_FOR(k, ng) gpos[gorder[k]] = (int)k;
}

// ---- stage 3 and the sorts by row ------------------------------------------------------------------
__global__ __launch_bounds__(kBlk) void k_gp(int P, const int *gid, const int *gpos, int *gp) {
    PLAN_FOR(p, P) gp[p] = gpos[gid[p]];
}

__global__ __launch_bounds__(kBlk) void k_count(int64_t n, const int *key, int *cnt) {
    PLAN_FOR(i, n) atomicAdd(&cnt[key[i]], 1);
}

__global__ __launch_bounds__(kBlk) void k_place(int64_t n, const int *key, const int *off, int *cur, int *out) {
    PLAN_FOR(i, n) {
        const int k = key[i];
        out[off[k] + atomicAdd(&cur[k], 1)] = (int)i;
    }
}

// every key's run in ascending order (an insertion sort by one thread; its cost follows the run's own length)
__global__ __launch_bounds__(kBlk) void k_run_sort(int nkeys, const int *off, int *out, int *hdr) {
    PLAN_FOR(k, nkeys) {
        const int a = off[k], b = off[k + 1];
        if (b - a < 2) continue;
        if (b - a > kPlanRunMax) { hdr[kHdrBound] = 1; continue; }
        for (int i = a + 1; i < b; i++) {
            const int v = out[i];
            int j = i - 1;
            while (j >= a && out[j] > v) { out[j + 1] = out[j]; j--; }
            out[j + 1] = v;
        }
    }
}

__global__ __launch_bounds__(kBlk) void k_inverse(int64_t n, const int *perm, int *inv) {
    PLAN_FOR(i, n) inv[perm[i]] = (int)i;
}

// ---- stage 4: rotation numbering -------------------------------------------------------------------
__global__ __launch_bounds__(kBlk) void k_rv(int64_t nloc, const int *aid, const int2 *rot, int2 *rv) {
    PLAN_FOR(l, nloc) rv[l] = rot[aid[l]];
}

__global__ __launch_bounds__(kBlk) void k_first(int64_t npos, const int *rv, int *first) {
    PLAN_FOR(x, npos) atomicMin(&first[rv[x]], (int)x);
}

__global__ __launch_bounds__(kBlk) void k_rflag(int64_t npos, const int *rv, const int *first, int *flag) {
    PLAN_FOR(x, npos) flag[x] = first[rv[x]] == (int)x;
}

// num: the exclusive scan of the flags (npos + 1 entries)
__global__ __launch_bounds__(kBlk) void k_rot_write(int64_t npos, const int *rv, const int *first, const int *num, int *rot_ids,
                                                   int *arl, int *hdr) {
    PLAN_FOR(x, npos) {
        const int g = rv[x], f = first[g];
        arl[x] = num[f];
        if (f == (int)x) rot_ids[num[x]] = g;
        if (x == 0) hdr[kHdrNrot] = num[npos];
    }
}

// ---- stages 5 and 6: keys ----------------------------------------------------------------------------
__global__ __launch_bounds__(kBlk) void k_key_edge(int64_t n, const int *point, const int *rop, int *key) {
    PLAN_FOR(e, n) key[e] = rop[point[e]];
}

// x = le << 2 | k
__global__ __launch_bounds__(kBlk) void k_key_inc(int64_t n4, const int *aid, const int *ap, const int *rop, int *key) {
    PLAN_FOR(x, n4) key[x] = rop[ap[4 * (int64_t)aid[x >> 2] + (x & 3)]];
}

__global__ __launch_bounds__(kBlk) void k_widen(int64_t n, const int *in, int64_t *out) {
    PLAN_FOR(i, n) out[i] = in[i];
}

}  // namespace dev

unsigned grid_for(int64_t n, int per_block = kBlk) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(kGridMax, (n + per_block - 1) / per_block));
}

size_t pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

const bool g_timing = std::getenv("DEFTRI_PLAN_TIMING") != nullptr;

}  // namespace

#define LAUNCH(k, n, ...)                                                                            \
    do {                                                                                             \
        if ((n) > 0) hipLaunchKernelGGL(dev::k, dim3(grid_for(n)), dim3(kBlk), 0, st_, __VA_ARGS__); \
    } while (0)

PlanDevice::~PlanDevice() {
    if (!buf_ && !pin_ && !ev_[0]) return;
    hipSetDevice(dev_);
    if (buf_) hipFree(buf_);
    if (pin_) hipHostFree(pin_);
    for (hipEvent_t e : ev_) if (e) hipEventDestroy(e);
}

bool PlanDevice::reserve(size_t dev_bytes, size_t pin_bytes, std::function<void()> *before_alloc) {
    if (!ev_[0])
        for (hipEvent_t &e : ev_) if (hipEventCreate(&e) != hipSuccess) return false;
    if ((dev_bytes > cap_ || pin_bytes > pin_cap_) && before_alloc && *before_alloc) {
        (*before_alloc)();
        *before_alloc = nullptr;
    }
    if (dev_bytes > cap_) {
        if (buf_) hipFree(buf_);
        buf_ = nullptr; cap_ = 0;
        const size_t want = dev_bytes + dev_bytes / 4;
        if (hipMalloc((void **)&buf_, want) != hipSuccess) return false;
        cap_ = want;
    }
    if (pin_bytes > pin_cap_) {
        if (pin_) hipHostFree(pin_);
        pin_ = nullptr; pin_cap_ = 0;
        const size_t want = pin_bytes + pin_bytes / 4;
        if (hipHostMalloc((void **)&pin_, want, hipHostMallocDefault) != hipSuccess) return false;
        pin_cap_ = want;
    }
    return true;
}

// the exclusive scan of data [n] in place: reduce / scan of the tile sums / apply, or one launch for one tile
void PlanDevice::scan(int *data, int64_t n) {
    if (n <= 0) return;
    const int ntile = (int)((n + kPlanScanTile - 1) / kPlanScanTile);
    int *part = (int *)(buf_ + L_.part);
    const dim3 grid((unsigned)std::min(ntile, kGridMax));
    if (ntile > 1) {
        hipLaunchKernelGGL(dev::k_scan_reduce, grid, dim3(kBlk), 0, st_, n, data, part, ntile);
        hipLaunchKernelGGL(dev::k_scan_part, dim3(1), dim3(1024), 0, st_, ntile, part);
    }
    hipLaunchKernelGGL(dev::k_scan_apply, grid, dim3(kBlk), 0, st_, n, data, ntile > 1 ? part : nullptr, ntile);
}

// out: the items 0 .. n - 1 sorted by (key, item); off [nkeys + 1]: the keys' offsets
void PlanDevice::sort_by_row(int64_t n, const int *key, int32_t nkeys, int *off, int *out, int *hdr) {
    hipMemsetAsync(off, 0, sizeof(int) * ((size_t)nkeys + 1), st_);
    if (n <= 0) return;
    int *cur = (int *)(buf_ + L_.cur);
    hipMemsetAsync(cur, 0, sizeof(int) * (size_t)nkeys, st_);
    LAUNCH(k_count, n, n, key, off);
    scan(off, (int64_t)nkeys + 1);
    LAUNCH(k_place, n, n, key, (const int *)off, cur, out);
    LAUNCH(k_run_sort, nkeys, nkeys, (const int *)off, out, hdr);
}

void PlanDevice::report(int first, int last, const char *const *names) const {
    if (!g_timing) return;
    for (int k = first; k < last; k++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev_[k], ev_[k + 1]) == hipSuccess)
            std::fprintf(stderr, "[deftri plan] %-28s %8.2f ms\n", names[k - first], ms);
    }
}

int PlanDevice::rows(const deftri_problem_desc &d, std::function<void()> *before_alloc, int32_t &ng,
                     std::vector<int32_t> &point_of_row, std::vector<int32_t> &row_of_point, std::vector<int32_t> &gp,
                     std::string &err) {
    hipSetDevice(dev_);
    const int32_t P = d.n_points, NR = std::max(d.n_rot, 1);
    const int64_t E = d.n_arap, R = d.n_rep, D = d.n_depth;
    const size_t Pz = (size_t)P, Ez = (size_t)E;
    const int stride = d.order_xy ? 2 : 3;
    const double *xy = d.order_xy ? d.order_xy : d.points;
    const int rtile = (int)((Pz + kPlanRadixTile - 1) / kPlanRadixTile);
    const int mm_grid = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (P + kBlk - 1) / kBlk));
    const int64_t scan_max = std::max<int64_t>({(int64_t)P + 1, (int64_t)kRadixDigits * rtile, 2 * E + 1});
    const size_t n_rot_cap = (size_t)std::min<int64_t>(NR, 2 * E);
    {
        size_t o = 0;
        auto piece = [&](size_t bytes) { const size_t at = o; o += pad(bytes); return at; };
        Layout &L = L_;
        L.ap = piece(16 * Ez); L.rot = piece(8 * Ez); L.rep_point = piece(4 * (size_t)R); L.dep_point = piece(4 * (size_t)D);
        L.xy = piece(8 * (size_t)stride * Pz);
        L.par = piece(4 * Pz); L.root = piece(4 * Pz); L.flag = piece(4 * (Pz + 1)); L.gid = piece(4 * Pz); L.grep = piece(4 * Pz);
        L.mm = piece(32 * (size_t)mm_grid); L.lohi = piece(32);
        L.key[0] = piece(8 * Pz); L.key[1] = piece(8 * Pz); L.id[0] = piece(4 * Pz); L.id[1] = piece(4 * Pz);
        L.hist = piece(4 * (size_t)kRadixDigits * rtile); L.gpos = piece(4 * Pz); L.cur = piece(4 * (Pz + 1));
        L.part = piece(4 * (size_t)((scan_max + kPlanScanTile - 1) / kPlanScanTile + 1));
        L.dl1 = o;                                          // the first download: one region
        L.hdr = piece(4 * kHdrWords); L.por = piece(4 * Pz); L.rop = piece(4 * Pz); L.gp = piece(4 * Pz);
        L.dl1_end = o;
        L.aid = piece(4 * Ez); L.rv = piece(8 * Ez); L.first = piece(4 * (size_t)NR); L.rflag = piece(4 * (2 * Ez + 1));
        L.kr = piece(4 * (size_t)R); L.kd = piece(4 * (size_t)D); L.ki = piece(16 * Ez); L.ioff = piece(4 * (Pz + 1));
        L.dl2 = o;                                          // the second download: one region
        L.hdr2 = piece(4 * kHdrWords); L.rot_ids = piece(4 * n_rot_cap); L.arl = piece(8 * Ez);
        L.rep_ids = piece(4 * (size_t)R); L.rep_off = piece(4 * (Pz + 1)); L.dep_ids = piece(4 * (size_t)D);
        L.dep_off = piece(4 * (Pz + 1)); L.inc = piece(16 * Ez); L.inc_off = piece(8 * (Pz + 1));
        L.dl2_end = o;
        L.total = o;
    }
    const Layout &L = L_;
    P_ = P; E_ = E;
    if (!reserve(L.total, std::max(L.dl1_end - L.dl1, L.dl2_end - L.dl2), before_alloc)) {
        err = "plan builder: allocation failed";
        return -1;
    }
    char *B = buf_;
    int *d_ap = (int *)(B + L.ap), *d_par = (int *)(B + L.par), *d_root = (int *)(B + L.root), *d_flag = (int *)(B + L.flag),
        *d_gid = (int *)(B + L.gid), *d_grep = (int *)(B + L.grep), *d_hist = (int *)(B + L.hist), *d_gpos = (int *)(B + L.gpos),
        *d_hdr = (int *)(B + L.hdr), *d_por = (int *)(B + L.por), *d_rop = (int *)(B + L.rop), *d_gp = (int *)(B + L.gp);
    double *d_xy = (double *)(B + L.xy), *d_mm = (double *)(B + L.mm), *d_lohi = (double *)(B + L.lohi);
    uint64_t *d_key[2] = {(uint64_t *)(B + L.key[0]), (uint64_t *)(B + L.key[1])};
    int *d_id[2] = {(int *)(B + L.id[0]), (int *)(B + L.id[1])};
    const int *d_ng = d_hdr + kHdrNg;

    // one upload of the inputs
    hipEventRecord(ev_[0], st_);
    hipMemcpyAsync(d_ap, d.arap_pts, 16 * Ez, hipMemcpyHostToDevice, st_);
    hipMemcpyAsync(B + L.rot, d.arap_rot, 8 * Ez, hipMemcpyHostToDevice, st_);
    if (R > 0) hipMemcpyAsync(B + L.rep_point, d.rep_point, 4 * (size_t)R, hipMemcpyHostToDevice, st_);
    if (D > 0) hipMemcpyAsync(B + L.dep_point, d.dep_point, 4 * (size_t)D, hipMemcpyHostToDevice, st_);
    hipMemcpyAsync(d_xy, xy, 8 * (size_t)stride * Pz, hipMemcpyHostToDevice, st_);
    hipEventRecord(ev_[1], st_);
    // 1. groups
    hipMemsetAsync(d_hdr, 0, 4 * kHdrWords, st_);
    hipMemsetAsync(d_flag + P, 0, 4, st_);
    LAUNCH(k_iota, P, (int64_t)P, d_par);
    LAUNCH(k_uf_hook, E, E, (const int4 *)d_ap, d_par, P, d_hdr);
    LAUNCH(k_uf_flatten, P, P, d_par, d_root, d_flag, d_hdr);
    scan(d_flag, (int64_t)P + 1);
    LAUNCH(k_groups, P, P, (const int *)d_root, (const int *)d_flag, d_gid, d_grep, d_hdr);
    hipEventRecord(ev_[2], st_);
    // 2. Morton order (ng stays on the device: the launches are sized by P, the kernels read ng)
    hipLaunchKernelGGL(dev::k_minmax_part, dim3(mm_grid), dim3(kBlk), 0, st_, d_ng, (const int *)d_grep, (const double *)d_xy, stride,
                       d_mm);
    hipLaunchKernelGGL(dev::k_minmax_final, dim3(1), dim3(kBlk), 0, st_, mm_grid, (const double *)d_mm, d_lohi);
    LAUNCH(k_keys, P, d_ng, (const int *)d_grep, (const double *)d_xy, stride, (const double *)d_lohi, d_key[0], d_id[0]);
    int cur = 0;
    const dim3 rgrid((unsigned)std::min(rtile, kGridMax));
    for (int pass = 0; pass < kRadixPasses; pass++) {
        const int sh = kPlanRadixBits * pass;
        hipLaunchKernelGGL(dev::k_radix_hist, rgrid, dim3(kBlk), 0, st_, d_ng, (const uint64_t *)d_key[cur], sh, d_hist, rtile);
        scan(d_hist, (int64_t)kRadixDigits * rtile);
        hipLaunchKernelGGL(dev::k_radix_scatter, rgrid, dim3(kBlk), 0, st_, d_ng, (const uint64_t *)d_key[cur],
                           (const int *)d_id[cur], sh, (const int *)d_hist, rtile, d_key[cur ^ 1], d_id[cur ^ 1]);
        cur ^= 1;
    }
    LAUNCH(k_gpos, P, d_ng, (const int *)d_id[cur], d_gpos);
    hipEventRecord(ev_[3], st_);
    // 3. rows: the points by (gpos[gid[p]], p)
    LAUNCH(k_gp, P, P, (const int *)d_gid, (const int *)d_gpos, d_gp);
    int *d_start = d_flag;                                  // the groups' offsets (P + 1: keys past ng are empty)
    sort_by_row(P, d_gp, P, d_start, d_por, d_hdr);
    LAUNCH(k_inverse, P, (int64_t)P, (const int *)d_por, d_rop);
    hipEventRecord(ev_[4], st_);
    hipMemcpyAsync(pin_, B + L.dl1, L.dl1_end - L.dl1, hipMemcpyDeviceToHost, st_);
    hipEventRecord(ev_[5], st_);
    hipError_t e = hipStreamSynchronize(st_);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
        err = std::string("plan builder (rows): ") + hipGetErrorString(e);
        return -1;
    }
    static const char *const names[] = {"dev upload inputs", "dev 1 groups (union-find)", "dev 2 Morton order", "dev 3 rows",
                                        "dev download rows"};
    report(0, 5, names);
    const int *hdr = (const int *)(pin_ + (L.hdr - L.dl1));
    if (hdr[kHdrBound]) return 1;
    ng = hdr[kHdrNg];
    if (ng < 0 || ng > P) {
        err = "plan builder: the device wrote an impossible group count";
        return -1;
    }
    const int32_t *por = (const int32_t *)(pin_ + (L.por - L.dl1)), *rop = (const int32_t *)(pin_ + (L.rop - L.dl1)),
                  *gpp = (const int32_t *)(pin_ + (L.gp - L.dl1));
    point_of_row.assign(por, por + P);
    row_of_point.assign(rop, rop + P);
    gp.assign(gpp, gpp + P);
    return 0;
}

int PlanDevice::edges(const deftri_problem_desc &d, SpPlanHost &H, std::string &err) {
    hipSetDevice(dev_);
    const Layout &L = L_;
    const int32_t P = P_, NR = std::max(d.n_rot, 1);
    const int64_t E = E_, R = d.n_rep, D = d.n_depth;
    const int64_t nloc = (int64_t)H.arap_ids.size(), npos = 2 * nloc, n4 = 4 * nloc;
    if (!buf_ || P != d.n_points || E != d.n_arap || nloc > E) {
        err = "plan builder: edges() without the rows of this problem";
        return -1;
    }
    for (int32_t e : H.arap_ids)
        if (e < 0 || e >= E) { err = "plan builder: a local edge id out of range"; return -1; }
    char *B = buf_;
    int *d_ap = (int *)(B + L.ap), *d_rep_point = (int *)(B + L.rep_point), *d_dep_point = (int *)(B + L.dep_point),
        *d_rop = (int *)(B + L.rop), *d_aid = (int *)(B + L.aid), *d_rv = (int *)(B + L.rv), *d_first = (int *)(B + L.first),
        *d_rflag = (int *)(B + L.rflag), *d_kr = (int *)(B + L.kr), *d_kd = (int *)(B + L.kd), *d_ki = (int *)(B + L.ki),
        *d_ioff = (int *)(B + L.ioff), *d_hdr = (int *)(B + L.hdr2), *d_rot_ids = (int *)(B + L.rot_ids), *d_arl = (int *)(B + L.arl),
        *d_rep_ids = (int *)(B + L.rep_ids), *d_rep_off = (int *)(B + L.rep_off), *d_dep_ids = (int *)(B + L.dep_ids),
        *d_dep_off = (int *)(B + L.dep_off), *d_inc = (int *)(B + L.inc);
    int64_t *d_inc_off = (int64_t *)(B + L.inc_off);

    hipEventRecord(ev_[6], st_);
    hipMemcpyAsync(d_aid, H.arap_ids.data(), 4 * (size_t)nloc, hipMemcpyHostToDevice, st_);
    hipEventRecord(ev_[7], st_);
    // 4. rotation rows numbered in first-encounter order over the positions 2 le + k
    hipMemsetAsync(d_hdr, 0, 4 * kHdrWords, st_);
    hipMemsetAsync(d_rflag + npos, 0, 4, st_);
    LAUNCH(k_rv, nloc, nloc, (const int *)d_aid, (const int2 *)(B + L.rot), (int2 *)d_rv);
    LAUNCH(k_fill, NR, (int64_t)NR, d_first, INT_MAX);
    LAUNCH(k_first, npos, npos, (const int *)d_rv, d_first);
    LAUNCH(k_rflag, npos, npos, (const int *)d_rv, (const int *)d_first, d_rflag);
    scan(d_rflag, npos + 1);
    LAUNCH(k_rot_write, npos, npos, (const int *)d_rv, (const int *)d_first, (const int *)d_rflag, d_rot_ids, d_arl, d_hdr);
    hipEventRecord(ev_[8], st_);
    // 5. reprojection / depth edges by row
    LAUNCH(k_key_edge, R, R, (const int *)d_rep_point, (const int *)d_rop, d_kr);
    sort_by_row(R, d_kr, P, d_rep_off, d_rep_ids, d_hdr);
    LAUNCH(k_key_edge, D, D, (const int *)d_dep_point, (const int *)d_rop, d_kd);
    sort_by_row(D, d_kd, P, d_dep_off, d_dep_ids, d_hdr);
    hipEventRecord(ev_[9], st_);
    // 6. incidences le << 2 | role by row
    LAUNCH(k_key_inc, n4, n4, (const int *)d_aid, (const int *)d_ap, (const int *)d_rop, d_ki);
    sort_by_row(n4, d_ki, P, d_ioff, d_inc, d_hdr);
    LAUNCH(k_widen, (int64_t)P + 1, (int64_t)P + 1, (const int *)d_ioff, d_inc_off);
    hipEventRecord(ev_[10], st_);
    hipMemcpyAsync(pin_, B + L.dl2, L.dl2_end - L.dl2, hipMemcpyDeviceToHost, st_);
    hipEventRecord(ev_[11], st_);
    hipError_t e = hipStreamSynchronize(st_);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
        err = std::string("plan builder (edges): ") + hipGetErrorString(e);
        return -1;
    }
    static const char *const names[] = {"dev upload arap_ids", "dev 5 rotation numbering", "dev 6 rep / depth by row",
                                        "dev 8 incidences", "dev download edges"};
    report(6, 11, names);
    auto at = [&](size_t off) { return pin_ + (off - L.dl2); };
    const int *hdr = (const int *)at(L.hdr2);
    if (hdr[kHdrBound]) return 1;
    const int nrot = nloc > 0 ? hdr[kHdrNrot] : 0;
    if (nrot < 0 || nrot > std::min<int64_t>(NR, npos)) {
        err = "plan builder: the device wrote an impossible rotation count";
        return -1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    auto take = [&](auto &v, size_t off, size_t n) {
        using T = typename std::remove_reference<decltype(v)>::type::value_type;
        const T *p = (const T *)at(off);
        v.assign(p, p + n);
    };
    take(H.rot_ids, L.rot_ids, (size_t)nrot);
    take(H.arap_rot_local, L.arl, (size_t)npos);
    take(H.rep_ids, L.rep_ids, (size_t)R);
    take(H.rep_off, L.rep_off, (size_t)P + 1);
    take(H.dep_ids, L.dep_ids, (size_t)D);
    take(H.dep_off, L.dep_off, (size_t)P + 1);
    take(H.inc, L.inc, (size_t)n4);
    take(H.inc_off, L.inc_off, (size_t)P + 1);
    if (g_timing) std::fprintf(stderr, "[deftri plan] %-28s %8.2f ms\n", "dev staging -> plan arrays", ms_since(t0));
    return 0;
}

}  // namespace deftri
