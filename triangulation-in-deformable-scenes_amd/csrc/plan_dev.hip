// plan_dev.hip — the one-pair tile plan's sorts, scans and numberings on the device (plan_dev.h), and
// its tile layout (build_tiles of one rank), its phase-1 blocks and its phase-2 wave layout (§5m); for
// several pairs the keyframe-major rows, with the same edge stages and wave layout after them (§5o), and their tile
// layout over (pair, group) units (build_tiles_multi, §5p).  Both tile layouts are cut by cut_tiles(), over groups or
// over units.
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

#include "dev_arena.h"
#include "spcg.h"

namespace deftri {

namespace {

constexpr int kBlk = 256;                 // threads per workgroup of the element-wise kernels
constexpr int kGridMax = 1 << 16;         // workgroups per launch at most; the rest is strided
constexpr int kRadixDigits = 1 << kPlanRadixBits;
constexpr int kRadixPasses = 42 / kPlanRadixBits;
static_assert(kRadixPasses * kPlanRadixBits == 42, "the passes cover the curve key exactly");
static_assert(kPlanScanTile == 8 * kBlk && kPlanRadixTile == kBlk, "one workgroup per tile");
enum { kHdrBound = 0, kHdrNg = 1, kHdrNrot = 2, kHdrWords = 16,
       // the tile stages' header: a condition build_tiles refuses, tiles, padded entries, halo rows, cut entries
       kHdrRefuse = 3, kHdrNt = 4, kHdrEntries = 5, kHdrHalo = 6, kHdrCut = 7, kHdrSegmax = 8, kHdrLds = 9,
       // the layout stages' header (stages 7 and 8b): waves, slot steps
       kLhNw = 4, kLhSlots = 5,
       // the rows of several pairs: a point with two cameras (the group order stays), the point count for the sort
       kHdrManyCam = 10, kHdrP = 11,
       // the tile layout of several pairs: the units, the share planes
       kHdrNu = 12, kHdrPlanes = 13 };

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

// ---- stage 3 of several pairs: the rows keyframe-major (spcg_plan.cpp) ---------------------
// a double as an integer of the same order (finite values; -0 below +0), and back
__device__ inline unsigned long long box_enc(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return b >> 63 ? ~b : b | 1ull << 63;
}

__device__ inline double box_dec(unsigned long long u) {
    return __longlong_as_double((long long)(u >> 63 ? u & ~(1ull << 63) : ~u));
}

// first[p]: the smallest reprojection edge at point p (INT_MAX: none)
__global__ __launch_bounds__(kBlk) void k_rep_first(int64_t R, const int *rep_point, int *first) {
    PLAN_FOR(e, R) atomicMin(&first[rep_point[e]], (int)e);
}

// one_cam is false when an edge names another camera than the first edge of its point
__global__ __launch_bounds__(kBlk) void k_cam_check(int64_t R, const int *rep_point, const int *rep_cam, const int *first, int *hdr) {
    PLAN_FOR(e, R)
        if (rep_cam[first[rep_point[e]]] != rep_cam[e]) hdr[kHdrManyCam] = 1;
}

// box [4 (C + 1)]: per camera lo x, lo y (to be minimised), hi x, hi y (maximised), encoded
__global__ __launch_bounds__(kBlk) void k_box_init(int n4, unsigned long long *box) {
    PLAN_FOR(i, n4) box[i] = box_enc((i & 3) < 2 ? 1e300 : -1e300);
}

// cam(p) = the camera of p's first edge, C without one; its box takes p's finite coordinates.  An integer atomic
// minimum / maximum gives the same result in any order; a thread whose value does not pass the word it reads
// (a stale word is only ever looser) leaves the atomic out
__global__ __launch_bounds__(kBlk) void k_cam_box(int P, int C, const int *first, const int *rep_cam, const double *pts, int stride,
                                                 int *pcam, unsigned long long *box) {
    PLAN_FOR(p, P) {
        const int f = first[p], cam = f == INT_MAX ? C : rep_cam[f];
        pcam[p] = cam;
        for (int c = 0; c < 2; c++) {
            const double v = pts[(int64_t)stride * p + c];
            if (!isfinite(v)) continue;
            const unsigned long long u = box_enc(v);
            unsigned long long *lo = box + 4 * (int64_t)cam + c, *hi = lo + 2;
            if (u < __hip_atomic_load(lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(lo, u);
            if (u > __hip_atomic_load(hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(hi, u);
        }
    }
}

// key = cam << 42 | curve_key of the point's own position in its camera's box; id = p, ascending
__global__ __launch_bounds__(kBlk) void k_cam_keys(int P, const int *pcam, const double *pts, int stride, const unsigned long long *box,
                                                  uint64_t *key, int *id) {
    PLAN_FOR(p, P) {
        const int cam = pcam[p];
        const unsigned long long *b = box + 4 * (int64_t)cam;
        const double lo[2] = {box_dec(b[0]), box_dec(b[1])}, hi[2] = {box_dec(b[2]), box_dec(b[3])};
        const double *q = pts + (int64_t)stride * p;
        key[p] = (uint64_t)cam << 42 | curve_key(q[0], q[1], lo, hi);
        id[p] = (int)p;
    }
}

// the rows are the sorted points unless the flag word chose the group order, which por already holds
__global__ __launch_bounds__(kBlk) void k_rows_pick(int P, const int *hdr, const int *sorted, int *por) {
    if (hdr[kHdrManyCam]) return;
    PLAN_FOR(r, P) por[r] = sorted[r];
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

// ---- the tile layout (build_tiles of one rank, spcg_tile.cpp) ----------------------------
// hdr: the tile stages' header.  A kernel that finds a condition build_tiles refuses sets kHdrRefuse; every later
// kernel returns at once when the header holds a refusal or a reached bound, so none of them sees a group of more
// than 2 rows, an edge inside one group, more than 64 out-edges or more than kPlanRunMax in-edges of a group.
// start: the groups' first rows (stage 3's offsets; the rows of a group are consecutive), P for the keys past ng
__device__ inline bool tile_stop(const int *hdr) { return (hdr[kHdrBound] | hdr[kHdrRefuse]) != 0; }

__global__ __launch_bounds__(kBlk) void k_tile_groups(int ng, const int *start, int *hdr) {
    PLAN_FOR(g, ng) if (start[g + 1] - start[g] > 2) hdr[kHdrRefuse] = 1;
}

__global__ __launch_bounds__(kBlk) void k_tile_edges(int64_t E, const int4 *ap, const int *gp, const int *rop, int *egi, int *egj,
                                                    int4 *erow, int *hdr) {
    PLAN_FOR(e, E) {
        const int4 v = ap[e];
        const int gi = gp[v.x], gj = gp[v.z];
        egi[e] = gi;
        egj[e] = gj;
        erow[e] = make_int4(rop[v.x], rop[v.y], rop[v.z], rop[v.w]);
        if (gi != gp[v.y] || gj != gp[v.w] || gi == gj) hdr[kHdrRefuse] = 1;
    }
}

__global__ __launch_bounds__(kBlk) void k_tile_deg(int ng, const int *ooff, int *hdr) {
    PLAN_FOR(g, ng) if (ooff[g + 1] - ooff[g] > 64) hdr[kHdrRefuse] = 1;
}

// per out-edge k (the order (gi, e)): its j group, and pred: the largest group below gi with an out-edge to the
// same gj, gi itself when an earlier edge of gi goes there, else -1.  An edge is the first of the groups [a, gi]
// to reach gj exactly when pred < a.  ie: the in-edges of a group, by (gj, e)
__global__ __launch_bounds__(kBlk) void k_tile_pred(int64_t E, const int *oe, const int *egi, const int *egj, const int *ioff,
                                                   const int *ie, int *okj, int *pred, const int *hdr) {
    if (tile_stop(hdr)) return;
    PLAN_FOR(k, E) {
        const int e = oe[k], gi = egi[e], gj = egj[e];
        int p = -1;
        const int a = ioff[gj], b = min(ioff[gj + 1], a + kPlanRunMax);
        for (int x = a; x < b; x++) {
            const int f = ie[x], gf = egi[f];
            if (gf < gi) p = max(p, gf);
            else if (gf == gi && f < e) p = gi;
        }
        okj[k] = gj;
        pred[k] = p;
    }
}

// the greedy cut from every start: tend[gs] = the first group the tile begun at gs does not take (build_tiles'
// loop; whether [gs, g] fits is a function of that set of groups alone).  At most umax + 1 steps.  upair (several
// pairs, else null): the units' pairs — a tile ends with its pair
__global__ __launch_bounds__(kBlk) void k_tile_end(int ng, const int *start, const int *ooff, const int *okj, const int *pred,
                                                  const int *ioff, const int *ie, const int *egi, int umax, int budget, int fixed,
                                                  int *tend, const int *hdr, const int *upair) {
    if (tile_stop(hdr)) return;
    PLAN_FOR(gs64, (int64_t)ng + 1) {
        const int gs = (int)gs64;
        if (gs == ng) { tend[gs] = ng; continue; }
        int nr = 0, nh = 0, ns = 0, units = 0, g = gs;
        for (int step = 0; step <= umax && g < ng; step++) {
            if (upair && upair[g] != upair[gs]) break;
            const int sz = start[g + 1] - start[g];
            int dnh = 0, dns = 0;
            bool was_halo = false;
            for (int k = ooff[g]; k < ooff[g + 1]; k++) {
                const int gj = okj[k];
                if (gj >= gs && gj < g) dns += 2;
                else if (pred[k] < gs) dnh += start[gj + 1] - start[gj];
            }
            for (int x = ioff[g]; x < ioff[g + 1]; x++) {
                const int gi = egi[ie[x]];
                if (gi >= gs && gi < g) { dns += 2; was_halo = true; }
            }
            if (was_halo) dnh -= sz;
            const bool fits = units + 1 <= umax && 24 * (nr + sz + nh + dnh) + 24 * (nr + sz) + 24 * (ns + dns) + fixed <= budget &&
                              nr + sz + nh + dnh < 4096 && ns + dns < 4096;
            if (!fits && units > 0) break;
            nr += sz; nh += dnh; ns += dns;
            units++;
            g++;
        }
        tend[gs] = g;
    }
}

// one round of pointer doubling over the nodes 0 .. ng: jin = end^(2^r).  A marked node marks its jin; every mark
// is on the chain 0, end(0), end(end(0)), ... whichever round's marks a thread happens to see
__global__ __launch_bounds__(kBlk) void k_tile_jump(int64_t n, const int *jin, int *jout, int *mark, const int *hdr) {
    if (tile_stop(hdr)) return;
    PLAN_FOR(g, n) {
        const int j = jin[g];
        if (mark[g]) mark[j] = 1;
        jout[g] = jin[j];
    }
}

__global__ __launch_bounds__(kBlk) void k_tile_midx(int ng, const int *mark, int *midx) {
    PLAN_FOR(g, (int64_t)ng + 1) midx[g] = g < ng ? mark[g] : 0;
}

// midx: the exclusive scan of the marks (ng + 1 entries)
__global__ __launch_bounds__(kBlk) void k_tile_tstart(int ng, const int *mark, const int *midx, int *tstart, int *hdr) {
    if (tile_stop(hdr)) return;
    PLAN_FOR(g, (int64_t)ng + 1) {
        if (g == ng) { tstart[midx[ng]] = ng; hdr[kHdrNt] = midx[ng]; }
        else if (mark[g]) tstart[midx[g]] = (int)g;
    }
}

// the entries of a tile's groups under the chunk rule (a unit never straddles a 64-entry chunk), by one thread:
// gst[i] = the first entry of group g0 + i inside the tile; returns the padded entry count, *segmax the longest unit
__device__ inline int tile_entry_layout(int g0, int g1, const int *ooff, int *gst, int *segmax) {
    int fill = 0, sm = 1;
    for (int g = g0; g < g1 && g - g0 < 128; g++) {
        const int cnt = ooff[g + 1] - ooff[g];
        if (cnt > 0 && fill % 64 + cnt > 64) fill = (fill + 63) & ~63;
        if (gst) gst[g - g0] = fill;
        fill += cnt;
        sm = max(sm, cnt);
    }
    *segmax = sm;
    return fill == 0 ? 64 : (fill + 63) & ~63;
}

// per tile: padded entries, halo rows, cut entries; segmax and the LDS maximum
__global__ __launch_bounds__(kBlk) void k_tile_count(const int *tstart, const int *start, const int *ooff, const int *okj,
                                                    const int *pred, int fixed, int *tne, int *tnh, int *tcut, int *hdr) {
    __shared__ int s_cut, s_nh;
    if (tile_stop(hdr)) return;
    const int nt = hdr[kHdrNt];
    for (int t = blockIdx.x; t < nt; t += gridDim.x) {
        const int g0 = tstart[t], g1 = tstart[t + 1], k0 = ooff[g0], k1 = ooff[g1];
        if (threadIdx.x == 0) { s_cut = 0; s_nh = 0; }
        __syncthreads();
        int cut = 0, nh = 0;
        for (int k = k0 + threadIdx.x; k < k1; k += blockDim.x) {
            const int gj = okj[k];
            if (gj < g0 || gj >= g1) {
                cut++;
                if (pred[k] < g0) nh += start[gj + 1] - start[gj];
            }
        }
        if (cut) atomicAdd(&s_cut, cut);
        if (nh) atomicAdd(&s_nh, nh);
        __syncthreads();
        if (threadIdx.x == 0) {
            int segmax;
            const int ne = tile_entry_layout(g0, g1, ooff, nullptr, &segmax);
            const int nr = start[g1] - start[g0], ns = 2 * (k1 - k0 - s_cut);
            tne[t] = ne;
            tnh[t] = s_nh;
            tcut[t] = s_cut;
            atomicMax(&hdr[kHdrSegmax], segmax);
            atomicMax(&hdr[kHdrLds], 24 * (nr + s_nh) + 24 * nr + 24 * ns + fixed);
            if (g1 - g0 > 128 || nr > 256) hdr[kHdrBound] = 1;      // (never: the cut takes at most 128 groups of 2 rows)
        }
        __syncthreads();
    }
}

// tne, tnh, tcut: exclusive scans over ng + 1 entries (zeros past nt), so entry ng holds the total
__global__ void k_tile_totals(int ng, const int *tne, const int *tnh, const int *tcut, int *hdr) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hdr[kHdrEntries] = tne[ng];
        hdr[kHdrHalo] = tnh[ng];
        hdr[kHdrCut] = tcut[ng];
    }
}

constexpr int kTileHaloMax = 4096;      // halo groups of one tile at most (rows + halo rows < 4096)

struct TileOut {
    int *tab, *chunk, *rs, *halo, *xrow;
    uint32_t *m0, *m1;
};

// one workgroup per tile: build_tiles' second stage as :338-468 writes it.  tne, tnh, tcut: the tiles' bases.
// Several pairs (urow, upair not null; build_tiles_multi's :781-866): a group is a unit, start[u] = 2 u, a row is its
// place 2 u + c in the tile row list (erow holds those), and urow gives the plan's row for the halo list and the cross
// slots' targets; the tile's pair goes to the table
__global__ __launch_bounds__(kBlk) void k_tile_fill(const int *tstart, const int *start, const int *gp, const int *por,
                                                   const int *ooff, const int *oe, const int *okj, const int *pred, const int *ioff,
                                                   const int *ie, const int *egi, const int4 *erow, const int *tne, const int *tnh,
                                                   const int *tcut, TileOut o, int *hdr, const int *hdr_in, const int *urow,
                                                   const int *upair) {
    __shared__ int hl[kTileHaloMax], hs[kTileHaloMax], ho[kTileHaloMax];   // halo groups << 2 | rows: found, sorted; row offsets
    __shared__ int gst[128], rsb[kBlk], sc[kBlk];
    __shared__ int s_hn, s_ne;
    if (tile_stop(hdr_in)) return;
    const int nt = hdr_in[kHdrNt];
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < nt; t += gridDim.x) {
        const int g0 = tstart[t], g1 = tstart[t + 1], k0 = ooff[g0], k1 = ooff[g1];
        const int r0 = start[g0], nr = start[g1] - r0;
        const int e0 = tne[t], h0 = tnh[t], x0 = 2 * tcut[t];
        if (tid == 0) {
            int segmax;
            s_ne = tile_entry_layout(g0, g1, ooff, gst, &segmax);
            s_hn = 0;
        }
        __syncthreads();
        const int ne = s_ne;
        // every entry a padding entry first (its own empty segment); the valid ones are written after the barrier
        for (int i = tid; i < ne; i += kBlk) { o.m0[e0 + i] = kTmHead; o.m1[e0 + i] = 0; }
        // the halo groups: the first out-edge of the tile to each group outside it
        for (int k = k0 + tid; k < k1; k += kBlk) {
            const int gj = okj[k];
            if ((gj < g0 || gj >= g1) && pred[k] < g0) {
                const int i = atomicAdd(&s_hn, 1);
                if (i < kTileHaloMax) hl[i] = gj << 2 | (start[gj + 1] - start[gj]);
            }
        }
        __syncthreads();
        const int hn = s_hn;
        if (hn > kTileHaloMax) {                          // (never: the partition keeps rows + halo rows below 4096)
            if (tid == 0) hdr[kHdrBound] = 1;
            __syncthreads();
            continue;
        }
        // ascending and unique: a group's place is the number of smaller ones, its first LDS row their rows
        for (int i = tid; i < hn; i += kBlk) {
            const int v = hl[i];
            int r = 0, rows = 0;
            for (int j = 0; j < hn; j++) {
                const int u = hl[j];
                if (u < v) { r++; rows += u & 3; }
            }
            hs[r] = v;
            ho[r] = rows;
        }
        // the own rows' slot counts: the in-edges of the row's group from the tile's groups that aim at the row
        int cnt = 0;
        if (tid < nr) {
            const int R = r0 + tid, g = urow ? R >> 1 : gp[por[R]];
            for (int x = ioff[g]; x < ioff[g + 1]; x++) {
                const int f = ie[x], gf = egi[f];
                if (gf >= g0 && gf < g1) {
                    const int4 w = erow[f];
                    cnt += (w.z == R) + (w.w == R);
                }
            }
        }
        int ns;
        const int sb = block_excl_scan(cnt, sc, &ns);     // (its barriers order hs / ho and the padding stores too)
        rsb[tid] = sb;
        if (tid < nr) {
            o.rs[r0 + tid] = sb | cnt << 16;
            if (cnt > 0xffff) hdr[kHdrRefuse] = 1;        // (never: a group has at most kPlanRunMax in-edges)
        }
        __syncthreads();
        int nh = 0;
        if (hn > 0) nh = ho[hn - 1] + (hs[hn - 1] & 3);
        for (int r = tid; r < hn; r += kBlk) {
            const int gj = hs[r] >> 2, sz = hs[r] & 3;
            for (int c = 0; c < sz; c++) o.halo[h0 + ho[r] + c] = urow ? urow[start[gj] + c] : start[gj] + c;
        }
        // the entries, 256 consecutive out-edges at a time: the cut entries before each are a scan with a carry
        int carry = 0;
        for (int kb = k0; kb < k1; kb += kBlk) {
            const int k = kb + tid;
            const bool valid = k < k1;
            int gj = 0;
            bool cut = false;
            if (valid) { gj = okj[k]; cut = gj < g0 || gj >= g1; }
            int tot;
            const int before = carry + block_excl_scan(cut ? 1 : 0, sc, &tot);
            carry += tot;
            if (!valid) continue;
            const int e = oe[k], g = egi[e];
            const int4 w = erow[e];
            const int pos = gst[g - g0] + (k - ooff[g]);
            const int ub = start[g] - r0;
            uint32_t w0 = kTmValid, w1 = (uint32_t)ub << 24;
            if (w.x - r0 == ub + 1) w0 |= kTmSwap;
            if (k == ooff[g]) w0 |= kTmHead;
            if (k == ooff[g + 1] - 1) w0 |= kTmLast;
            if (cut) {
                int lo = 0, hi = hn;                      // the place of gj among the halo groups
                const int key = gj << 2;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if ((hs[mid] & ~3) < key) lo = mid + 1; else hi = mid;
                }
                lo = min(lo, hn - 1);                     // (gj is among them: some edge of the tile was the first to reach it)
                const int lrow = nr + ho[lo] - start[gj];
                w0 |= (uint32_t)(lrow + w.z) | (uint32_t)(lrow + w.w) << 12 | kTmCut;
                const int x = x0 + 2 * before;
                o.xrow[x] = urow ? urow[w.z] : w.z;
                o.xrow[x + 1] = urow ? urow[w.w] : w.w;
            } else {
                // the slot an in-tile entry takes on a row of j: its rank among the (entry, which) aimed at that
                // row in entry order — the order (gi, e), then p1_j before p2_j
                int rk0 = 0, rk1 = 0;
                for (int x = ioff[gj]; x < ioff[gj + 1]; x++) {
                    const int f = ie[x], gf = egi[f];
                    if (gf < g0 || gf >= g1) continue;
                    const int4 v = erow[f];
                    const bool earlier = gf < g || (gf == g && f < e);
                    if (earlier) {
                        rk0 += (v.z == w.z) + (v.w == w.z);
                        rk1 += (v.z == w.w) + (v.w == w.w);
                    } else if (f == e) {
                        rk1 += w.z == w.w;
                    }
                }
                const int s0 = rsb[w.z - r0] + rk0, s1 = rsb[w.w - r0] + rk1;
                w0 |= (uint32_t)(w.z - r0) | (uint32_t)(w.w - r0) << 12;
                w1 |= (uint32_t)s0 | (uint32_t)s1 << 12;
            }
            o.m0[e0 + pos] = w0;
            o.m1[e0 + pos] = w1;
            if (pos % 64 == 0) {
                o.chunk[2 * ((e0 + pos) / 64)] = k;
                o.chunk[2 * ((e0 + pos) / 64) + 1] = x0 + 2 * before;
            }
        }
        if (tid == 0) {
            if (k0 == k1) { o.chunk[2 * (e0 / 64)] = k0; o.chunk[2 * (e0 / 64) + 1] = x0; }
            int *T = o.tab + 8 * (int64_t)t;
            T[0] = r0; T[1] = nr; T[2] = nh; T[3] = e0; T[4] = ne; T[5] = h0; T[6] = ns; T[7] = upair ? upair[g0] : 0;
        }
        __syncthreads();
    }
}

// ---- the tile layout of several pairs (build_tiles_multi, spcg_tile.cpp) -------------------
// A unit is a (pair q, group g) some edge end touches, flat index k = q ng + g.  Its flag is an idempotent store; its
// points (the p1 copy upt, the p2 copy upt2) are the smallest any end names — on a graph build_tiles_multi accepts
// every end names the same two, and k_mu_edges refuses one where an end does not
__global__ __launch_bounds__(kBlk) void k_mu_flag(int64_t E, const int4 *ap, const int *pair, const int *gp, int Q, int ng, int *uflag,
                                                 int *upt, int *upt2, int *hdr) {
    PLAN_FOR(e, E) {
        const int q = pair[e];
        if (q < 0 || q >= Q) { hdr[kHdrRefuse] = 1; continue; }
        const int4 v = ap[e];
        const int ki = q * ng + gp[v.x], kj = q * ng + gp[v.z];
        uflag[ki] = 1;
        uflag[kj] = 1;
        atomicMin(&upt[ki], v.x);
        atomicMin(&upt2[ki], v.y);
        atomicMin(&upt[kj], v.z);
        atomicMin(&upt2[kj], v.w);
    }
}

// per pair the box of its units' points (box [4 Q] as k_box_init leaves it; the atomics as in k_cam_box)
__global__ __launch_bounds__(kBlk) void k_mu_box(int nU, int ng, const int *uflag, const int *upt, const double *pts,
                                                unsigned long long *box) {
    PLAN_FOR(k, nU) {
        if (!uflag[k]) continue;
        const int q = (int)k / ng;
        for (int c = 0; c < 2; c++) {
            const unsigned long long u = box_enc(pts[3 * (int64_t)upt[k] + c]);
            unsigned long long *lo = box + 4 * (int64_t)q + c, *hi = lo + 2;
            if (u < __hip_atomic_load(lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(lo, u);
            if (u > __hip_atomic_load(hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(hi, u);
        }
    }
}

// uidx: the exclusive scan of the flags (nU + 1 entries), the units' numbers in ascending (q, g).  key = q << 42 | the
// curve key of the unit's point in its pair's box, id = k
__global__ __launch_bounds__(kBlk) void k_mu_keys(int nU, int ng, const int *uflag, const int *uidx, const int *upt, const double *pts,
                                                 const unsigned long long *box, uint64_t *key, int *id, int *hdr) {
    PLAN_FOR(k, nU) {
        if (k == 0) hdr[kHdrNu] = uidx[nU];
        if (!uflag[k]) continue;
        const int q = (int)k / ng;
        const unsigned long long *b = box + 4 * (int64_t)q;
        const double lo[2] = {box_dec(b[0]), box_dec(b[1])}, hi[2] = {box_dec(b[2]), box_dec(b[3])};
        const double *pp = pts + 3 * (int64_t)upt[k];
        key[uidx[k]] = (uint64_t)q << 42 | curve_key(pp[0], pp[1], lo, hi);
        id[uidx[k]] = (int)k;
    }
}

// ids: the units in their order (q, key, g).  uid [nU] (filled with -1 before), the units' rows and pairs, and
// ustart[u] = 2 u for u <= nmax + 1 — the "groups' first rows" the one-pair kernels read
__global__ __launch_bounds__(kBlk) void k_mu_units(int nmax, int ng, const int *ids, const int *upt, const int *upt2, const int *rop,
                                                  int *uid, int *urow, int *upair, int *ustart, const int *hdr) {
    const int nu = min(hdr[kHdrNu], nmax);
    PLAN_FOR(u, (int64_t)nmax + 2) {
        ustart[u] = 2 * (int)u;
        if (u >= nu) continue;
        const int k = ids[u];
        uid[k] = (int)u;
        urow[2 * u] = rop[upt[k]];
        urow[2 * u + 1] = rop[upt2[k]];
        upair[u] = k / ng;
    }
}

// per edge its units, and its four rows as places 2 u + c in the tile row list.  Refused: an edge inside one unit, an
// edge's copies in two groups, an end that names another point than its unit's
__global__ __launch_bounds__(kBlk) void k_mu_edges(int64_t E, const int4 *ap, const int *pair, const int *gp, int Q, int ng,
                                                  const int *uid, const int *upt, const int *upt2, int *egi, int *egj, int4 *erow,
                                                  int *hdr) {
    PLAN_FOR(e, E) {
        const int q = pair[e];
        const int4 v = ap[e];
        int ui = 0, uj = 0;
        bool bad = q < 0 || q >= Q;
        if (!bad) {
            const int ki = q * ng + gp[v.x], kj = q * ng + gp[v.z];
            ui = uid[ki];
            uj = uid[kj];
            bad = ui == uj || ui < 0 || uj < 0 || gp[v.y] != gp[v.x] || gp[v.w] != gp[v.z] || upt[ki] != v.x || upt2[ki] != v.y ||
                  upt[kj] != v.z || upt2[kj] != v.w;
        }
        if (bad) { hdr[kHdrRefuse] = 1; ui = uj = 0; }
        egi[e] = ui;
        egj[e] = uj;
        erow[e] = make_int4(2 * ui, 2 * ui + 1, 2 * uj, 2 * uj + 1);
    }
}

// every depth edge's (row, pair of its scale) is a row of that pair's unit of its group
__global__ __launch_bounds__(kBlk) void k_mu_depth(int64_t D, const int *dep_point, const int *dscale, const int *gp, const int *rop,
                                                  int Q, int ng, const int *uid, const int *urow, int *hdr) {
    PLAN_FOR(x, D) {
        const int p = dep_point[x], q = dscale[x] >> 1;
        const int u = q >= 0 && q < Q ? uid[q * ng + gp[p]] : -1;
        if (u < 0 || (urow[2 * u] != rop[p] && urow[2 * u + 1] != rop[p])) hdr[kHdrRefuse] = 1;
    }
}

// soff: the offsets of the tile row list's entries by row.  A row in no unit is refused; the share planes
__global__ __launch_bounds__(kBlk) void k_mu_rows(int P, const int *soff, int *hdr) {
    PLAN_FOR(r, P) {
        const int c = soff[r + 1] - soff[r];
        if (c == 0) hdr[kHdrRefuse] = 1;
        else if (c - 1 > hdr[kHdrPlanes]) atomicMax(&hdr[kHdrPlanes], c - 1);
    }
}

// spos: the place of entry k in the sort by (row, k).  Its share is its rank among its row's entries; share 0 is home
__global__ __launch_bounds__(kBlk) void k_mu_shares(int64_t n2, const int *urow, const int *soff, const int *spos, int *trow, int *tdst) {
    PLAN_FOR(k, n2) {
        const int r = urow[k], j = spos[k] - soff[r];
        tdst[k] = j;
        trow[k] = j == 0 ? r | (int)(1u << 31) : r;
    }
}

__global__ __launch_bounds__(kBlk) void k_mu_nshare(int P, const int *soff, int *nshare) {
    PLAN_FOR(r, P) nshare[r] = soff[r + 1] - soff[r];
}

// poff[q]: the first tile at or after pair q's first unit — uidx[q ng] units come before the pair, midx (the scan of
// the tile starts' marks) counts the tiles that start before a unit; poff[Q] is the tile count
__global__ __launch_bounds__(kBlk) void k_mu_poff(int Q, int ng, const int *uidx, const int *midx, int *poff) {
    PLAN_FOR(q, (int64_t)Q + 1) poff[q] = midx[uidx[q * ng]];
}

// ---- stages 7 and 8b: phase-1 blocks and the phase-2 wave layout (spcg_plan.cpp) ---------------
// One rank, one pair, at most two scales: every local ARAP edge has heavy vertex 0, the local depth edges are all
// of them, a local row is its global row.  hdr: the layout's header (the words k_tile_jump reads stay 0)

// flag [D + 1]: depth edge j (in dep_ids order) is of scale 0; its exclusive scan places the scale-0 edges
__global__ __launch_bounds__(kBlk) void k_dep_flag(int D, const int *dep_ids, const int *dscale, int *flag) {
    PLAN_FOR(j, (int64_t)D + 1) flag[j] = j < D ? dscale[dep_ids[j]] == 0 : 0;
}

// dperm: the local depth edges sorted stably by scale — scale 0 in order, then the rest in order (n0 = pos0[D])
__global__ __launch_bounds__(kBlk) void k_dperm(int D, const int *dep_ids, const int *dscale, const int *pos0, int *dperm) {
    const int n0 = pos0[D];
    PLAN_FOR(j, D) {
        const int p = pos0[j];
        dperm[dscale[dep_ids[j]] == 0 ? p : n0 + ((int)j - p)] = (int)j;
    }
}

// the blocks in the host's order of creation — owned ARAP, halo-only ARAP, depth scale 0, depth scale 1, each in
// runs of kSpBlock — and each block's key, the row of its first edge's point
__global__ __launch_bounds__(kBlk) void k_blk_make(int nb, int nao, int nloc, int n0, int D, const int *aid, const int *ap,
                                                  const int *rop, const int *dep_point, const int *dep_ids, const int *dperm,
                                                  const int *dscale, int4 *blk0, int *bkey) {
    const int nb0 = (nao + kSpBlock - 1) / kSpBlock, nb1 = nb0 + (nloc - nao + kSpBlock - 1) / kSpBlock,
              nb2 = nb1 + (n0 + kSpBlock - 1) / kSpBlock;
    PLAN_FOR(b, nb) {
        int kind = SP_ARAP, owned = 1, lo = 0, hi = nao, k = (int)b;
        if (b >= nb2) { kind = SP_DEP; lo = n0; hi = D; k = (int)b - nb2; }
        else if (b >= nb1) { kind = SP_DEP; hi = n0; k = (int)b - nb1; }
        else if (b >= nb0) { owned = 0; lo = nao; hi = nloc; k = (int)b - nb0; }
        const int begin = lo + k * kSpBlock, end = min(hi, begin + kSpBlock);
        int hv = 0, key;
        if (kind == SP_ARAP) key = rop[ap[4 * (int64_t)aid[begin]]];
        else {
            const int e = dep_ids[dperm[begin]];
            hv = dscale[e];
            key = rop[dep_point[e]];
        }
        blk0[b] = make_int4(kind | owned << 8, hv, begin, end);
        bkey[b] = key;
    }
}

// the dispatch order: sorted block s = x seg + j (segment x's j-th block) goes to the position it has in the
// host's list "for j, for x: if x seg + j < nb" — the rows j' < j hold q + 1 blocks while j' <= r, else q
__global__ __launch_bounds__(kBlk) void k_blk_deal(int nb, const int *bord, const int4 *blk0, int4 *blk) {
    const int seg = (nb + 7) / 8, q = (nb - 1) / seg, r = (nb - 1) % seg;
    PLAN_FOR(s, nb) {
        const int x = (int)s / seg, j = (int)s % seg;
        const int64_t pos = (int64_t)j * (q + 1) - max(0, j - r - 1) + x;
        blk[pos] = blk0[bord[s]];
    }
}

// hv_blk_off / hv_blk: per heavy vertex (nlist = Q + S <= 3) its blocks in final block order, by one workgroup
__global__ __launch_bounds__(1024) void k_blk_heavy(int nb, int nlist, const int4 *blk, int *hvb, int *hvoff) {
    __shared__ int s[1024];
    int base = 0;
    for (int h = 0; h < nlist && h < 3; h++) {
        if (threadIdx.x == 0) hvoff[h] = base;
        int carry = 0;
        for (int b0 = 0; b0 < nb; b0 += 1024) {
            const int b = b0 + threadIdx.x;
            int f = 0;
            if (b < nb) {
                const int4 v = blk[b];
                const int heavy = (v.x & 0xff) == SP_ARAP ? ((v.x >> 8) ? v.y : -1) : 1 + v.y;
                f = heavy == h;
            }
            int tot;
            const int ex = block_excl_scan(f, s, &tot);
            if (f) hvb[base + carry + ex] = b;
            carry += tot;
        }
        base += carry;
    }
    if (threadIdx.x == 0) hvoff[nlist] = base;
}

__device__ inline int row_slots(int l, const int *ioff, const int *doff) { return ioff[l + 1] - ioff[l] + doff[l + 1] - doff[l]; }

// the rows of every window of kSpSortWindow by slot count, descending and stable: a row's place is the number of
// larger counts plus the equal counts before it (one workgroup per window, one thread per row)
__global__ __launch_bounds__(kSpSortWindow) void k_win_sort(int P, int nwin, const int *ioff, const int *doff, int *order, int *scnt) {
    __shared__ int c[kSpSortWindow];
    for (int w = blockIdx.x; w < nwin; w += gridDim.x) {
        const int w0 = w * kSpSortWindow, n = min(kSpSortWindow, P - w0), t = threadIdx.x;
        const int mine = t < n ? row_slots(w0 + t, ioff, doff) : -1;
        c[t] = mine;
        __syncthreads();
        if (t < n) {
            int rank = 0;
            for (int u = 0; u < n; u++) {
                const int v = c[u];
                rank += (v > mine) | ((v == mine) & (u < t));
            }
            order[w0 + rank] = w0 + t;
            scnt[w0 + rank] = mine;
        }
        __syncthreads();
    }
}

// a wave starting at sorted row 32 g: split when the next 64 rows (to P, across windows) hold a count above
// kSpWaveSplit; its steps from the rows it takes; the next wave's node.  Node ni ends the chain
__global__ __launch_bounds__(kBlk) void k_wave_cut(int P, int ni, const int *scnt, int *wnext, int *wsteps, int *wsp) {
    PLAN_FOR(g, (int64_t)ni + 1) {
        if (g == ni) { wnext[g] = ni; wsteps[g] = 0; wsp[g] = 0; continue; }
        const int i = 32 * (int)g;
        int kmax = 0;
        for (int j = 0; j < 64 && i + j < P; j++) kmax = max(kmax, scnt[i + j]);
        const int sp = kSpWaveSplit > 0 && kmax > kSpWaveSplit;
        const int nr = sp ? 32 : 64;
        int steps = 0;
        for (int j = 0; j < nr && i + j < P; j++) {
            const int c = scnt[i + j];
            steps = max(steps, sp ? (c + 1) / 2 : c);
        }
        wnext[g] = min(ni, (int)g + nr / 32);
        wsteps[g] = steps;
        wsp[g] = sp;
    }
}

// the marked nodes are the waves: widx their flags, wsoff their steps (both ni + 1 entries, then scanned)
__global__ __launch_bounds__(kBlk) void k_wave_marks(int ni, const int *mark, const int *wsteps, int *widx, int *wsoff) {
    PLAN_FOR(g, (int64_t)ni + 1) {
        const int m = g < ni && mark[g];
        widx[g] = m;
        wsoff[g] = m ? wsteps[g] : 0;
    }
}

// rowmap, wsplit and woff of every wave (x = node << 6 | lane), the wave count and the slot steps
__global__ __launch_bounds__(kBlk) void k_wave_write(int P, int ni, const int *mark, const int *widx, const int *wsoff, const int *wsp,
                                                    const int *order, int *rowmap, int *woff, uint8_t *wsplit, int *hdr) {
    PLAN_FOR(x, 64 * (int64_t)ni) {
        if (x == 0) {
            const int nw = widx[ni];
            woff[nw] = wsoff[ni];
            hdr[kLhNw] = nw;
            hdr[kLhSlots] = wsoff[ni];
        }
        const int g = (int)(x >> 6), j = (int)(x & 63);
        if (!mark[g]) continue;
        const int w = widx[g], sp = wsp[g], i = 32 * g;
        rowmap[64 * (int64_t)w + j] = j < (sp ? 32 : 64) && i + j < P ? order[i + j] : -1;
        if (j == 0) { wsplit[w] = (uint8_t)sp; woff[w] = wsoff[g]; }
    }
}

// one thread per (wave, lane) writes its row's slot list into the -1-filled pmap / pidx: the ARAP incidences, then
// the depth couplings; a split row's second half goes to lane j + 32.  nsl: the slot steps (the arrays hold 64 nsl)
__global__ __launch_bounds__(kBlk) void k_slot_fill(int nw, int nsl, const int *rowmap, const int *woff, const uint8_t *wsplit,
                                                   const int *ioff, const int *inc, const int *doff, const int *dep_ids,
                                                   const int *dscale, int *pmap, int *pidx, int *hdr) {
    PLAN_FOR(x, 64 * (int64_t)nw) {
        const int w = (int)(x >> 6), j = (int)(x & 63);
        const bool sp = wsplit[w] != 0;
        if (j >= (sp ? 32 : 64)) continue;
        const int l = rowmap[x];
        if (l < 0) continue;
        const int a0 = ioff[l], na = ioff[l + 1] - a0, b0 = doff[l], size = na + doff[l + 1] - b0;
        const int h = sp ? (size + 1) / 2 : size, base = woff[w];
        if (size > 2 * kPlanRunMax || base + h > nsl) { hdr[kHdrBound] = 1; continue; }
        for (int t = 0; t < size; t++) {
            int pm, pi;
            if (t < na) { pm = inc[a0 + t]; pi = pm >> 2; }
            else { const int xd = b0 + t - na; pm = -(2 + xd); pi = -(2 + dscale[dep_ids[xd]]); }
            const int64_t at = 64 * (int64_t)(base + (t < h ? t : t - h)) + (t < h ? j : j + 32);
            pmap[at] = pm;
            pidx[at] = pi;
        }
    }
}

}  // namespace dev

unsigned grid_for(int64_t n, int per_block = kBlk) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(kGridMax, (n + per_block - 1) / per_block));
}

size_t pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

const bool g_timing = std::getenv("DEFTRI_PLAN_TIMING") != nullptr;

void call_once(std::function<void()> *before_alloc) {
    if (before_alloc && *before_alloc) {
        (*before_alloc)();
        *before_alloc = nullptr;
    }
}

// a grow-only device arena: at least want_bytes, a quarter more when it grows; before_alloc is called (and cleared) first
bool grow(char *&buf, size_t &cap, size_t want_bytes, std::function<void()> *before_alloc) {
    if (want_bytes <= cap) return true;
    call_once(before_alloc);
    if (buf) hipFree(buf);
    buf = nullptr; cap = 0;
    const size_t bytes = want_bytes + want_bytes / 4;
    if (hipMalloc((void **)&buf, bytes) != hipSuccess) return false;
    cap = bytes;
    return true;
}

// v = the n elements at base + offset of a download
template <class V>
void take(V &v, const char *base, size_t offset, size_t n) {
    const typename V::value_type *p = (const typename V::value_type *)(base + offset);
    v.assign(p, p + n);
}

}  // namespace

#define LAUNCH(k, n, ...)                                                                            \
    do {                                                                                             \
        if ((n) > 0) hipLaunchKernelGGL(dev::k, dim3(grid_for(n)), dim3(kBlk), 0, st_, __VA_ARGS__); \
    } while (0)

PlanDevice::~PlanDevice() {
    if (!buf_ && !pin_ && !tbuf_ && !sbuf_ && !mbuf_ && !ev_[0]) return;
    hipSetDevice(dev_);
    if (buf_) hipFree(buf_);
    if (tbuf_) hipFree(tbuf_);
    if (sbuf_) hipFree(sbuf_);
    if (mbuf_) hipFree(mbuf_);
    if (pin_) hipHostFree(pin_);
    for (hipEvent_t e : ev_) if (e) hipEventDestroy(e);
}

bool PlanDevice::reserve(size_t dev_bytes, size_t pin_bytes, std::function<void()> *before_alloc) {
    if (!ev_[0])
        for (hipEvent_t &e : ev_) if (hipEventCreate(&e) != hipSuccess) return false;
    if (!grow(buf_, cap_, dev_bytes, before_alloc)) return false;
    if (pin_bytes > pin_cap_) {
        call_once(before_alloc);
        if (pin_) hipHostFree(pin_);
        pin_ = nullptr; pin_cap_ = 0;
        const size_t want = pin_bytes + pin_bytes / 4;
        if (hipHostMalloc((void **)&pin_, want, hipHostMallocDefault) != hipSuccess) return false;
        pin_cap_ = want;
    }
    return true;
}

bool PlanDevice::sync(const char *what, std::string &err) {
    hipError_t e = hipStreamSynchronize(st_);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) return true;
    err = std::string("plan builder (") + what + "): " + hipGetErrorString(e);
    return false;
}

int PlanDevice::refuse(std::vector<int32_t> &gp, const char *what, std::string &err) {
    hipMemcpyAsync(pin_, buf_ + L_.gp, 4 * (size_t)P_, hipMemcpyDeviceToHost, st_);
    if (!sync(what, err)) return -1;
    gp.assign((const int32_t *)pin_, (const int32_t *)pin_ + P_);
    return 2;
}

// the exclusive scan of data [n] in place: reduce / scan of the tile sums / apply, or one launch for one tile
void PlanDevice::scan(int *data, int64_t n, int *part) {
    if (n <= 0) return;
    const int ntile = (int)((n + kPlanScanTile - 1) / kPlanScanTile);
    if (!part) part = (int *)(buf_ + L_.part);
    const dim3 grid((unsigned)std::min(ntile, kGridMax));
    if (ntile > 1) {
        hipLaunchKernelGGL(dev::k_scan_reduce, grid, dim3(kBlk), 0, st_, n, data, part, ntile);
        hipLaunchKernelGGL(dev::k_scan_part, dim3(1), dim3(1024), 0, st_, ntile, part);
    }
    hipLaunchKernelGGL(dev::k_scan_apply, grid, dim3(kBlk), 0, st_, n, data, ntile > 1 ? part : nullptr, ntile);
}

// out: the items 0 .. n - 1 sorted by (key, item); off [nkeys + 1]: the keys' offsets
void PlanDevice::sort_by_row(int64_t n, const int *key, int32_t nkeys, int *off, int *out, int *hdr, int *cur, int *part) {
    hipMemsetAsync(off, 0, sizeof(int) * ((size_t)nkeys + 1), st_);
    if (n <= 0) return;
    if (!cur) cur = (int *)(buf_ + L_.cur);
    hipMemsetAsync(cur, 0, sizeof(int) * (size_t)nkeys, st_);
    LAUNCH(k_count, n, n, key, off);
    scan(off, (int64_t)nkeys + 1, part);
    LAUNCH(k_place, n, n, key, (const int *)off, cur, out);
    LAUNCH(k_run_sort, nkeys, nkeys, (const int *)off, out, hdr);
}

// the stable LSD radix sort of the *np keys in key[0] / id[0] (ntile tiles of kPlanRadixTile hold them); returns the
// buffer that holds the result
int PlanDevice::radix_sort(uint64_t *const key[2], int *const id[2], int *hist, int *part, const int *np, int ntile, int passes) {
    const dim3 rgrid((unsigned)std::min(ntile, kGridMax));
    int cur = 0;
    for (int pass = 0; pass < passes; pass++) {
        const int sh = kPlanRadixBits * pass;
        hipLaunchKernelGGL(dev::k_radix_hist, rgrid, dim3(kBlk), 0, st_, np, (const uint64_t *)key[cur], sh, hist, ntile);
        scan(hist, (int64_t)kRadixDigits * ntile, part);
        hipLaunchKernelGGL(dev::k_radix_scatter, rgrid, dim3(kBlk), 0, st_, np, (const uint64_t *)key[cur], (const int *)id[cur], sh,
                           (const int *)hist, ntile, key[cur ^ 1], id[cur ^ 1]);
        cur ^= 1;
    }
    return cur;
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
                     std::string &err, PlanBuilders on) {
    hipSetDevice(dev_);
    on.multi_tiles = on.multi_tiles && on.multi;
    if (on.multi && (on.tiles || d.n_cams >= (1 << 21))) {
        err = "plan builder: rows() of several pairs with the tile stages, or with 2^21 cameras";
        return -1;
    }
    on_ = on;
    order_on_dev_ = false;
    nloc_ = -1;
    const int32_t P = d.n_points, NR = std::max(d.n_rot, 1);
    const int64_t E = d.n_arap, R = d.n_rep, D = d.n_depth;
    const size_t Pz = (size_t)P, Ez = (size_t)E;
    const int stride = d.order_xy ? 2 : 3;
    const double *xy = d.order_xy ? d.order_xy : d.points;
    const int rtile = (int)((Pz + kPlanRadixTile - 1) / kPlanRadixTile);
    const int mm_grid = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (P + kBlk - 1) / kBlk));
    const int64_t scan_max = std::max<int64_t>({(int64_t)P + 1, (int64_t)kRadixDigits * rtile, 2 * E + 1, D + 1});
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
        if (on.tiles) {
            L.egi = piece(4 * Ez); L.egj = piece(4 * Ez); L.erow = piece(16 * Ez); L.ooff = piece(4 * (Pz + 1)); L.oe = piece(4 * Ez);
            L.okj = piece(4 * Ez); L.pred = piece(4 * Ez); L.tioff = piece(4 * (Pz + 1)); L.ie = piece(4 * Ez);
            L.tend = piece(4 * (Pz + 1)); L.ja = piece(4 * (Pz + 1)); L.jb = piece(4 * (Pz + 1)); L.mark = piece(4 * (Pz + 2));
            L.midx = piece(4 * (Pz + 2)); L.tstart = piece(4 * (Pz + 2)); L.tne = piece(4 * (Pz + 2)); L.tnh = piece(4 * (Pz + 2));
            L.tcut = piece(4 * (Pz + 2)); L.thdr = piece(4 * kHdrWords);
        }
        L.dl3 = L.dl3_end = o;
        if (on.layout) {
            // at most nbm blocks, ni wave starts (every 32 rows) and as many waves; several pairs: stage 8b alone,
            // so stage 7's pieces (D7 depth edges, nbm blocks, P7 block keys) are empty
            const size_t ni = (Pz + 31) / 32, Dz = (size_t)D, D7 = on.multi ? 0 : Dz, P7 = on.multi ? 0 : Pz + 1;
            const size_t nbm = on.multi ? 0 : Ez / kSpBlock + (size_t)D / kSpBlock + 4;
            L.dscale = piece(4 * Dz); L.dflag = piece(4 * (D7 + 1)); L.bkey = piece(4 * nbm); L.boff = piece(4 * P7);
            L.bord = piece(4 * nbm); L.blk0 = piece(16 * nbm); L.order = piece(4 * Pz); L.scnt = piece(4 * Pz);
            L.wnext = piece(4 * (ni + 1)); L.wsteps = piece(4 * (ni + 1)); L.wsp = piece(4 * (ni + 1)); L.wja = piece(4 * (ni + 1));
            L.wjb = piece(4 * (ni + 1)); L.wmark = piece(4 * (ni + 1)); L.widx = piece(4 * (ni + 1)); L.wsoff = piece(4 * (ni + 1));
            L.dl3 = o;                                      // the layout's download: one region
            L.lhdr = piece(4 * kHdrWords); L.dperm = piece(4 * D7); L.blk = piece(16 * nbm); L.hvb = piece(4 * nbm);
            L.hvoff = piece(4 * 4); L.rowmap = piece(4 * 64 * ni); L.woff = piece(4 * (ni + 1)); L.wsplit = piece(ni);
            L.dl3_end = o;
        }
        L.pxy = L.rcam = L.rfirst = L.pcam = L.cbox = o;
        if (on.multi) {
            // the points' own coordinates (with order_xy: beside it), the edges' cameras, per point its first edge and
            // its camera, per camera (and the bucket without one) its box
            L.pxy = piece(d.order_xy ? 24 * Pz : 0); L.rcam = piece(4 * (size_t)R); L.rfirst = piece(4 * Pz); L.pcam = piece(4 * Pz);
            L.cbox = piece(32 * ((size_t)std::max(d.n_cams, 1) + 1));
        }
        L.mpair = L.mdscale = o;
        if (on.multi_tiles) {
            L.mpair = piece(4 * Ez);
            L.mdscale = on.layout ? L.dscale : piece(4 * (size_t)D);
        }
        L.total = o;
    }
    const Layout &L = L_;
    P_ = P; E_ = E;
    if (!reserve(L.total, std::max({L.dl1_end - L.dl1, L.dl2_end - L.dl2, L.dl3_end - L.dl3}), before_alloc)) {
        err = "plan builder: allocation failed";
        return -1;
    }
    if (g_timing)
        std::fprintf(stderr, "[deftri plan] arena %.1f MiB of %.1f, pinned staging %.1f MiB\n", L.total / 1048576.0, cap_ / 1048576.0,
                     pin_cap_ / 1048576.0);
    char *B = buf_;
    int *d_ap = (int *)(B + L.ap), *d_par = (int *)(B + L.par), *d_root = (int *)(B + L.root), *d_flag = (int *)(B + L.flag),
        *d_gid = (int *)(B + L.gid), *d_grep = (int *)(B + L.grep), *d_hist = (int *)(B + L.hist), *d_gpos = (int *)(B + L.gpos),
        *d_hdr = (int *)(B + L.hdr), *d_por = (int *)(B + L.por), *d_rop = (int *)(B + L.rop), *d_gp = (int *)(B + L.gp);
    double *d_xy = (double *)(B + L.xy), *d_mm = (double *)(B + L.mm), *d_lohi = (double *)(B + L.lohi);
    uint64_t *d_key[2] = {(uint64_t *)(B + L.key[0]), (uint64_t *)(B + L.key[1])};
    int *d_id[2] = {(int *)(B + L.id[0]), (int *)(B + L.id[1])};
    const int *d_ng = d_hdr + kHdrNg;

    // one upload of the inputs
    hipEventRecord(ev_[kEvRows], st_);
    hipMemcpyAsync(d_ap, d.arap_pts, 16 * Ez, hipMemcpyHostToDevice, st_);
    hipMemcpyAsync(B + L.rot, d.arap_rot, 8 * Ez, hipMemcpyHostToDevice, st_);
    if (R > 0) hipMemcpyAsync(B + L.rep_point, d.rep_point, 4 * (size_t)R, hipMemcpyHostToDevice, st_);
    if (D > 0) hipMemcpyAsync(B + L.dep_point, d.dep_point, 4 * (size_t)D, hipMemcpyHostToDevice, st_);
    hipMemcpyAsync(d_xy, xy, 8 * (size_t)stride * Pz, hipMemcpyHostToDevice, st_);
    if (on.layout && D > 0) hipMemcpyAsync(B + L.dscale, d.dep_scale, 4 * (size_t)D, hipMemcpyHostToDevice, st_);
    if (on.multi && R > 0) hipMemcpyAsync(B + L.rcam, d.rep_cam, 4 * (size_t)R, hipMemcpyHostToDevice, st_);
    if (on.multi && d.order_xy) hipMemcpyAsync(B + L.pxy, d.points, 24 * Pz, hipMemcpyHostToDevice, st_);
    if (on.multi_tiles) hipMemcpyAsync(B + L.mpair, d.arap_pair, 4 * Ez, hipMemcpyHostToDevice, st_);
    if (on.multi_tiles && !on.layout && D > 0) hipMemcpyAsync(B + L.mdscale, d.dep_scale, 4 * (size_t)D, hipMemcpyHostToDevice, st_);
    hipEventRecord(ev_[kEvRows + 1], st_);
    // 1. groups
    hipMemsetAsync(d_hdr, 0, 4 * kHdrWords, st_);
    hipMemsetAsync(d_flag + P, 0, 4, st_);
    LAUNCH(k_iota, P, (int64_t)P, d_par);
    LAUNCH(k_uf_hook, E, E, (const int4 *)d_ap, d_par, P, d_hdr);
    LAUNCH(k_uf_flatten, P, P, d_par, d_root, d_flag, d_hdr);
    scan(d_flag, (int64_t)P + 1);
    LAUNCH(k_groups, P, P, (const int *)d_root, (const int *)d_flag, d_gid, d_grep, d_hdr);
    hipEventRecord(ev_[kEvRows + 2], st_);
    // 2. Morton order (ng stays on the device: the launches are sized by P, the kernels read ng)
    hipLaunchKernelGGL(dev::k_minmax_part, dim3(mm_grid), dim3(kBlk), 0, st_, d_ng, (const int *)d_grep, (const double *)d_xy, stride,
                       d_mm);
    hipLaunchKernelGGL(dev::k_minmax_final, dim3(1), dim3(kBlk), 0, st_, mm_grid, (const double *)d_mm, d_lohi);
    LAUNCH(k_keys, P, d_ng, (const int *)d_grep, (const double *)d_xy, stride, (const double *)d_lohi, d_key[0], d_id[0]);
    int cur = radix_sort(d_key, d_id, d_hist, nullptr, d_ng, rtile, kRadixPasses);
    LAUNCH(k_gpos, P, d_ng, (const int *)d_id[cur], d_gpos);
    hipEventRecord(ev_[kEvRows + 3], st_);
    // 3. rows: the points by (gpos[gid[p]], p)
    LAUNCH(k_gp, P, P, (const int *)d_gid, (const int *)d_gpos, d_gp);
    int *d_start = d_flag;                                  // the groups' offsets (P + 1: keys past ng are empty)
    sort_by_row(P, d_gp, P, d_start, d_por, d_hdr);
    if (on.multi) {
        // several pairs: by (camera, curve key in the camera's box, point) instead, when every point has one camera.
        // The camera is the key's bits from 42 up: ceil(bits(C) / 7) more passes of the same sort
        const int C = std::max(d.n_cams, 1);
        int cbits = 0;
        while (C >> cbits) cbits++;
        const double *d_pts = d.order_xy ? (const double *)(B + L.pxy) : (const double *)d_xy;
        int *d_rcam = (int *)(B + L.rcam), *d_rfirst = (int *)(B + L.rfirst), *d_pcam = (int *)(B + L.pcam);
        unsigned long long *d_box = (unsigned long long *)(B + L.cbox);
        LAUNCH(k_fill, 1, (int64_t)1, d_hdr + kHdrP, P);
        LAUNCH(k_fill, P, (int64_t)P, d_rfirst, INT_MAX);
        LAUNCH(k_rep_first, R, R, (const int *)(B + L.rep_point), d_rfirst);
        LAUNCH(k_cam_check, R, R, (const int *)(B + L.rep_point), (const int *)d_rcam, (const int *)d_rfirst, d_hdr);
        LAUNCH(k_box_init, 4 * (C + 1), 4 * (C + 1), d_box);
        LAUNCH(k_cam_box, P, P, C, (const int *)d_rfirst, (const int *)d_rcam, d_pts, 3, d_pcam, d_box);
        LAUNCH(k_cam_keys, P, P, (const int *)d_pcam, d_pts, 3, (const unsigned long long *)d_box, d_key[0], d_id[0]);
        cur = radix_sort(d_key, d_id, d_hist, nullptr, d_hdr + kHdrP, rtile, kRadixPasses + (cbits + kPlanRadixBits - 1) / kPlanRadixBits);
        LAUNCH(k_rows_pick, P, P, (const int *)d_hdr, (const int *)d_id[cur], d_por);
    }
    LAUNCH(k_inverse, P, (int64_t)P, (const int *)d_por, d_rop);
    hipEventRecord(ev_[kEvRows + 4], st_);
    // (gp is the region's last piece: the tile stages read it on the device, so it stays there)
    hipMemcpyAsync(pin_, B + L.dl1, (on.tiles || on.multi_tiles ? L.gp : L.dl1_end) - L.dl1, hipMemcpyDeviceToHost, st_);
    hipEventRecord(ev_[kEvRows + 5], st_);
    if (!sync("rows", err)) return -1;
    static const char *const names[] = {"dev upload inputs", "dev 1 groups (union-find)", "dev 2 Morton order", "dev 3 rows",
                                        "dev download rows"};
    report(kEvRows, kEvRows + 5, names);
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
    if (on.tiles || on.multi_tiles) gp.clear();
    else gp.assign(gpp, gpp + P);
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

    nloc_ = -1;
    hipEventRecord(ev_[kEvEdges], st_);
    if (order_on_dev_ && nloc == E) hipMemcpyAsync(d_aid, order_dev_, 4 * (size_t)nloc, hipMemcpyDeviceToDevice, st_);
    else hipMemcpyAsync(d_aid, H.arap_ids.data(), 4 * (size_t)nloc, hipMemcpyHostToDevice, st_);
    hipEventRecord(ev_[kEvEdges + 1], st_);
    // 4. rotation rows numbered in first-encounter order over the positions 2 le + k
    hipMemsetAsync(d_hdr, 0, 4 * kHdrWords, st_);
    hipMemsetAsync(d_rflag + npos, 0, 4, st_);
    LAUNCH(k_rv, nloc, nloc, (const int *)d_aid, (const int2 *)(B + L.rot), (int2 *)d_rv);
    LAUNCH(k_fill, NR, (int64_t)NR, d_first, INT_MAX);
    LAUNCH(k_first, npos, npos, (const int *)d_rv, d_first);
    LAUNCH(k_rflag, npos, npos, (const int *)d_rv, (const int *)d_first, d_rflag);
    scan(d_rflag, npos + 1);
    LAUNCH(k_rot_write, npos, npos, (const int *)d_rv, (const int *)d_first, (const int *)d_rflag, d_rot_ids, d_arl, d_hdr);
    hipEventRecord(ev_[kEvEdges + 2], st_);
    // 5. reprojection / depth edges by row
    LAUNCH(k_key_edge, R, R, (const int *)d_rep_point, (const int *)d_rop, d_kr);
    sort_by_row(R, d_kr, P, d_rep_off, d_rep_ids, d_hdr);
    LAUNCH(k_key_edge, D, D, (const int *)d_dep_point, (const int *)d_rop, d_kd);
    sort_by_row(D, d_kd, P, d_dep_off, d_dep_ids, d_hdr);
    hipEventRecord(ev_[kEvEdges + 3], st_);
    // 6. incidences le << 2 | role by row
    LAUNCH(k_key_inc, n4, n4, (const int *)d_aid, (const int *)d_ap, (const int *)d_rop, d_ki);
    sort_by_row(n4, d_ki, P, d_ioff, d_inc, d_hdr);
    LAUNCH(k_widen, (int64_t)P + 1, (int64_t)P + 1, (const int *)d_ioff, d_inc_off);
    hipEventRecord(ev_[kEvEdges + 4], st_);
    hipMemcpyAsync(pin_, B + L.dl2, L.dl2_end - L.dl2, hipMemcpyDeviceToHost, st_);
    hipEventRecord(ev_[kEvEdges + 5], st_);
    if (!sync("edges", err)) return -1;
    static const char *const names[] = {"dev upload arap_ids", "dev 5 rotation numbering", "dev 6 rep / depth by row",
                                        "dev 8 incidences", "dev download edges"};
    report(kEvEdges, kEvEdges + 5, names);
    const int *hdr = (const int *)(pin_ + (L.hdr2 - L.dl2));
    if (hdr[kHdrBound]) return 1;
    const int nrot = nloc > 0 ? hdr[kHdrNrot] : 0;
    if (nrot < 0 || nrot > std::min<int64_t>(NR, npos)) {
        err = "plan builder: the device wrote an impossible rotation count";
        return -1;
    }
    const auto t0 = std::chrono::steady_clock::now();
    take(H.rot_ids, pin_, L.rot_ids - L.dl2, (size_t)nrot);
    take(H.arap_rot_local, pin_, L.arl - L.dl2, (size_t)npos);
    take(H.rep_ids, pin_, L.rep_ids - L.dl2, (size_t)R);
    take(H.rep_off, pin_, L.rep_off - L.dl2, (size_t)P + 1);
    take(H.dep_ids, pin_, L.dep_ids - L.dl2, (size_t)D);
    take(H.dep_off, pin_, L.dep_off - L.dl2, (size_t)P + 1);
    take(H.inc, pin_, L.inc - L.dl2, (size_t)n4);
    take(H.inc_off, pin_, L.inc_off - L.dl2, (size_t)P + 1);
    nloc_ = nloc;
    if (g_timing) std::fprintf(stderr, "[deftri plan] %-28s %8.2f ms\n", "dev staging -> plan arrays", ms_since(t0));
    return 0;
}

// cut_tiles(): its scratch on the device, over n nodes (groups, or units) and E edges
struct PlanDevice::TileScratch {
    int *hdr;                         // the stages' header: zeroed, then marked by the front end's kernels
    const int *start;                 // [n + 1] the nodes' first rows
    int *egi, *egj, *erow;            // per edge its two nodes and its four rows, written by the front end
    int *ooff, *oe, *okj, *pred, *ioff, *ie, *tend, *ja, *jb, *mark, *midx, *tstart, *tne, *tnh, *tcut;
    int *cur, *part;                  // the scratch of sort_by_row and scan (null: the arena's own pieces)
    const int *gp, *por;              // one pair: a tile's rows are its groups' points (else null)
    const int *urow, *upair;          // several pairs: the units' two rows and their pairs (else null)
};

// what a layout of several pairs adds to cut_tiles(): the depth edges' and the rows' checks and the tile row list's
// entries by (row, entry) before the partition; the shares, the rows' share counts and the pairs' tile offsets after
// the fill, four more arrays of the download
struct PlanDevice::MultiExtras {
    int32_t Q, ng;
    int64_t D;
    const int *dep_point, *dscale, *gp, *rop, *uid, *uidx;
    int *soff, *sk, *spos;
};

int PlanDevice::cut_tiles(const TileScratch &s, const MultiExtras *mx, int32_t n, int units_max, int lds_budget,
                          std::function<void()> *before_alloc, SpPlanHost &H, std::vector<int32_t> &order, std::vector<int32_t> &gp,
                          std::string &err) {
    const char *what = mx ? "tiles of several pairs" : "tiles";
    const int32_t P = P_;
    const int64_t E = E_, nodes = (int64_t)n + 1, n2 = mx ? 2 * (int64_t)n : 0;
    const size_t Pz = (size_t)P, Ez = (size_t)E;
    const dim3 tgrid((unsigned)std::min(n, kGridMax));
    // a. the edges by node: the out-edges by (ni, e), the in-edges by (nj, e)
    sort_by_row(E, s.egi, n, s.ooff, s.oe, s.hdr, s.cur, s.part);
    LAUNCH(k_tile_deg, n, n, (const int *)s.ooff, s.hdr);
    sort_by_row(E, s.egj, n, s.ioff, s.ie, s.hdr, s.cur, s.part);
    LAUNCH(k_tile_pred, E, E, (const int *)s.oe, (const int *)s.egi, (const int *)s.egj, (const int *)s.ioff, (const int *)s.ie, s.okj,
           s.pred, (const int *)s.hdr);
    if (mx) {
        LAUNCH(k_mu_depth, mx->D, mx->D, mx->dep_point, mx->dscale, mx->gp, mx->rop, mx->Q, mx->ng, mx->uid, s.urow, s.hdr);
        sort_by_row(n2, s.urow, P, mx->soff, mx->sk, s.hdr, s.cur, s.part);
        LAUNCH(k_inverse, n2, n2, (const int *)mx->sk, mx->spos);
        LAUNCH(k_mu_rows, P, P, (const int *)mx->soff, s.hdr);
    }
    hipEventRecord(ev_[kEvCut + 1], st_);
    // b. partition: the cut from every start (several pairs: a tile ends with its pair), the chain from node 0 marked
    // by pointer doubling and compacted
    LAUNCH(k_tile_end, nodes, n, s.start, (const int *)s.ooff, (const int *)s.okj, (const int *)s.pred, (const int *)s.ioff,
           (const int *)s.ie, (const int *)s.egi, units_max, lds_budget, (int)kSpTileLdsFixed, s.tend, (const int *)s.hdr, s.upair);
    hipMemsetAsync(s.mark, 0, 4 * ((size_t)n + 2), st_);
    LAUNCH(k_fill, 1, (int64_t)1, s.mark, 1);
    {
        int rounds = 1;
        while (((int64_t)1 << (rounds - 1)) < nodes) rounds++;
        const int *jin = s.tend;
        int *jout = s.ja;
        for (int r = 0; r < rounds; r++) {
            LAUNCH(k_tile_jump, nodes, nodes, jin, jout, s.mark, (const int *)s.hdr);
            jin = jout;
            jout = jout == s.ja ? s.jb : s.ja;
        }
    }
    LAUNCH(k_tile_midx, nodes, n, (const int *)s.mark, s.midx);
    scan(s.midx, nodes, s.part);
    LAUNCH(k_tile_tstart, nodes, n, (const int *)s.mark, (const int *)s.midx, s.tstart, s.hdr);
    hipEventRecord(ev_[kEvCut + 2], st_);
    // c (counts). per tile its padded entries, halo rows and cut entries; their scans are the tiles' bases
    hipMemsetAsync(s.tne, 0, 4 * ((size_t)n + 1), st_);
    hipMemsetAsync(s.tnh, 0, 4 * ((size_t)n + 1), st_);
    hipMemsetAsync(s.tcut, 0, 4 * ((size_t)n + 1), st_);
    hipLaunchKernelGGL(dev::k_tile_count, tgrid, dim3(kBlk), 0, st_, (const int *)s.tstart, s.start, (const int *)s.ooff,
                       (const int *)s.okj, (const int *)s.pred, (int)kSpTileLdsFixed, s.tne, s.tnh, s.tcut, s.hdr);
    scan(s.tne, nodes, s.part);
    scan(s.tnh, nodes, s.part);
    scan(s.tcut, nodes, s.part);
    hipLaunchKernelGGL(dev::k_tile_totals, dim3(1), dim3(64), 0, st_, n, (const int *)s.tne, (const int *)s.tnh, (const int *)s.tcut,
                       s.hdr);
    hipEventRecord(ev_[kEvCut + 3], st_);
    hipMemcpyAsync(pin_, s.hdr, 4 * kHdrWords, hipMemcpyDeviceToHost, st_);
    hipEventRecord(ev_[kEvCut + 4], st_);
    if (!sync(what, err)) return -1;
    static const char *const names1[] = {"dev 4a groups, edges by group", "dev 4a partition", "dev 4a tile counts", "dev download counts"};
    static const char *const names1m[] = {"dev 4a edges by unit, shares", "dev 4a partition", "dev 4a tile counts", "dev download counts"};
    report(kEvCut, kEvCut + 4, mx ? names1m : names1);
    int hdr[kHdrWords];
    std::memcpy(hdr, pin_, sizeof(hdr));
    // the host's builder refuses this graph (with its own reason): it runs there from these rows
    if (hdr[kHdrRefuse]) return refuse(gp, what, err);
    if (hdr[kHdrBound]) return 1;
    const int32_t nt = hdr[kHdrNt], planes = mx ? hdr[kHdrPlanes] : 0;
    const int64_t ne = hdr[kHdrEntries], nhr = hdr[kHdrHalo], nx = 2 * (int64_t)hdr[kHdrCut];
    if (nt < 1 || nt > n || ne < 64 * (int64_t)nt || ne % 64 || ne > 2 * E + 64 * (int64_t)nt || nhr < 0 || nhr > 2 * E || nx < 0 ||
        nx > 2 * E || (mx && (planes < 0 || planes >= mx->Q))) {
        err = "plan builder: the device wrote impossible tile counts";
        return -1;
    }
    // the tile arrays: one download region (header, tile arrays, the edge order, several pairs: their four arrays),
    // then the cross slots' scratch
    const size_t nrs = mx ? (size_t)n2 : Pz;                // tile_rs: per row, or the units' two rows
    size_t o = 0;
    auto piece = [&](size_t bytes) { const size_t at = o; o += pad(bytes); return at; };
    const size_t o_hdr = piece(4 * kHdrWords), o_tab = piece(32 * (size_t)nt), o_m0 = piece(4 * (size_t)ne), o_m1 = piece(4 * (size_t)ne),
                 o_chunk = piece(8 * (size_t)(ne / 64)), o_rs = piece(4 * nrs), o_halo = piece(4 * (size_t)nhr),
                 o_xoff = piece(4 * (Pz + 1)), o_xdst = piece(4 * (size_t)nx), o_order = piece(4 * Ez), o_trow = piece(4 * (size_t)n2),
                 o_tdst = piece(4 * (size_t)n2), o_poff = piece(mx ? 4 * ((size_t)mx->Q + 1) : 0), o_nshare = piece(mx ? 4 * Pz : 0);
    const size_t dl = o;
    const size_t o_xrow = piece(4 * (size_t)nx), o_xs = piece(4 * (size_t)nx);
    if (!grow(tbuf_, tcap_, o, before_alloc) || !reserve(cap_, dl, before_alloc)) { err = "plan builder: allocation failed"; return -1; }
    char *T = tbuf_;
    int *d_hdr3 = (int *)(T + o_hdr), *d_xoff = (int *)(T + o_xoff), *d_xdst = (int *)(T + o_xdst), *d_xs = (int *)(T + o_xs);
    dev::TileOut out;
    out.tab = (int *)(T + o_tab); out.chunk = (int *)(T + o_chunk); out.rs = (int *)(T + o_rs); out.halo = (int *)(T + o_halo);
    out.xrow = (int *)(T + o_xrow); out.m0 = (uint32_t *)(T + o_m0); out.m1 = (uint32_t *)(T + o_m1);
    hipEventRecord(ev_[kEvFill], st_);
    // c. entries and slots (several pairs: and own rows), one workgroup per tile; the shares from the sort by (row, entry)
    hipMemsetAsync(d_hdr3, 0, 4 * kHdrWords, st_);
    hipLaunchKernelGGL(dev::k_tile_fill, dim3((unsigned)std::min(nt, kGridMax)), dim3(kBlk), 0, st_, (const int *)s.tstart, s.start, s.gp,
                       s.por, (const int *)s.ooff, (const int *)s.oe, (const int *)s.okj, (const int *)s.pred, (const int *)s.ioff,
                       (const int *)s.ie, (const int *)s.egi, (const int4 *)s.erow, (const int *)s.tne, (const int *)s.tnh,
                       (const int *)s.tcut, out, d_hdr3, (const int *)s.hdr, s.urow, s.upair);
    if (mx) {
        LAUNCH(k_mu_shares, n2, n2, s.urow, (const int *)mx->soff, (const int *)mx->spos, (int *)(T + o_trow), (int *)(T + o_tdst));
        LAUNCH(k_mu_nshare, P, P, (const int *)mx->soff, (int *)(T + o_nshare));
        LAUNCH(k_mu_poff, (int64_t)mx->Q + 1, mx->Q, mx->ng, mx->uidx, (const int *)s.midx, (int *)(T + o_poff));
    }
    hipEventRecord(ev_[kEvFill + 1], st_);
    // d. cross slots by (target row, slot): a row's offsets, and every slot's place in that order
    sort_by_row(nx, out.xrow, P, d_xoff, d_xs, d_hdr3, s.cur, s.part);
    LAUNCH(k_inverse, nx, nx, (const int *)d_xs, d_xdst);
    hipMemcpyAsync(T + o_order, s.oe, 4 * Ez, hipMemcpyDeviceToDevice, st_);
    hipEventRecord(ev_[kEvFill + 2], st_);
    hipMemcpyAsync(pin_, T, dl, hipMemcpyDeviceToHost, st_);
    hipEventRecord(ev_[kEvFill + 3], st_);
    if (!sync(what, err)) return -1;
    static const char *const names2[] = {"dev 4a entries, slots", "dev 4a cross slots", "dev download tiles"};
    static const char *const names2m[] = {"dev 4a entries, slots, shares", "dev 4a cross slots", "dev download tiles"};
    report(kEvFill, kEvFill + 3, mx ? names2m : names2);
    const int *hdr3 = (const int *)(pin_ + o_hdr);
    if (hdr3[kHdrBound] || hdr3[kHdrRefuse]) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    take(H.tile_tab, pin_, o_tab, 8 * (size_t)nt);
    take(H.tile_m0, pin_, o_m0, (size_t)ne);
    take(H.tile_m1, pin_, o_m1, (size_t)ne);
    take(H.tile_chunk, pin_, o_chunk, 2 * (size_t)(ne / 64));
    take(H.tile_rs, pin_, o_rs, nrs);
    take(H.tile_halo, pin_, o_halo, (size_t)nhr);
    take(H.tile_xoff, pin_, o_xoff, Pz + 1);
    take(H.tile_xdst, pin_, o_xdst, (size_t)nx);
    take(order, pin_, o_order, Ez);
    if (mx) {
        take(H.tile_trow, pin_, o_trow, (size_t)n2);
        take(H.tile_tdst, pin_, o_tdst, (size_t)n2);
        take(H.tile_poff, pin_, o_poff, (size_t)mx->Q + 1);
        take(H.tile_nshare, pin_, o_nshare, Pz);
        H.tile_planes = planes;
        H.tile_multi = true;
    }
    H.ntile = nt;
    H.tile_entries = ne;
    H.tile_cross = nx;
    H.tile_segmax = std::max(1, hdr[kHdrSegmax]);
    H.tile_lds = hdr[kHdrLds];
    H.tile_halo_rows = nhr;
    order_on_dev_ = true;
    order_dev_ = s.oe;
    if (g_timing) std::fprintf(stderr, "[deftri plan] %-28s %8.2f ms\n", "dev staging -> tile arrays", ms_since(t0));
    return 0;
}

int PlanDevice::tiles(const deftri_problem_desc &d, int32_t ng, int units_max, int lds_budget, std::function<void()> *before_alloc,
                      SpPlanHost &H, std::vector<int32_t> &order, std::vector<int32_t> &gp, std::string &err) {
    hipSetDevice(dev_);
    const Layout &L = L_;
    const int32_t P = P_;
    const int64_t E = E_;
    if (!buf_ || !on_.tiles || P != d.n_points || E != d.n_arap || ng < 1 || ng > P) {
        err = "plan builder: tiles() without the rows of this problem";
        return -1;
    }
    char *B = buf_;
    auto ip = [&](size_t off) { return (int *)(B + off); };
    const int *d_ap = ip(L.ap), *d_rop = ip(L.rop);
    TileScratch s{};
    s.hdr = ip(L.thdr); s.start = ip(L.flag); s.egi = ip(L.egi); s.egj = ip(L.egj); s.erow = ip(L.erow); s.ooff = ip(L.ooff);
    s.oe = ip(L.oe); s.okj = ip(L.okj); s.pred = ip(L.pred); s.ioff = ip(L.tioff); s.ie = ip(L.ie); s.tend = ip(L.tend); s.ja = ip(L.ja);
    s.jb = ip(L.jb); s.mark = ip(L.mark); s.midx = ip(L.midx); s.tstart = ip(L.tstart); s.tne = ip(L.tne); s.tnh = ip(L.tnh);
    s.tcut = ip(L.tcut); s.gp = ip(L.gp); s.por = ip(L.por);

    hipEventRecord(ev_[kEvCut], st_);
    // the groups' checks, and per edge its groups and rows
    hipMemsetAsync(s.hdr, 0, 4 * kHdrWords, st_);
    LAUNCH(k_tile_groups, ng, ng, s.start, s.hdr);
    LAUNCH(k_tile_edges, E, E, (const int4 *)d_ap, s.gp, d_rop, s.egi, s.egj, (int4 *)s.erow, s.hdr);
    return cut_tiles(s, nullptr, ng, units_max, lds_budget, before_alloc, H, order, gp, err);
}

int PlanDevice::tiles_multi(const deftri_problem_desc &d, int32_t ng, int units_max, int lds_budget, std::function<void()> *before_alloc,
                            SpPlanHost &H, std::vector<int32_t> &order, std::vector<int32_t> &gp, std::string &err) {
    hipSetDevice(dev_);
    const Layout &L = L_;
    const int32_t P = P_, Q = d.n_pairs;
    const int64_t E = E_;
    const char *what = "tiles of several pairs";
    if (!buf_ || !on_.multi_tiles || P != d.n_points || E != d.n_arap || ng < 1 || ng > P || Q < 2 || E < 1) {
        err = "plan builder: tiles_multi() without the rows of this problem";
        return -1;
    }
    char *B = buf_;
    const int *d_ap = (const int *)(B + L.ap), *d_gp = (const int *)(B + L.gp), *d_rop = (const int *)(B + L.rop),
              *d_pair = (const int *)(B + L.mpair);
    const double *d_pts = d.order_xy ? (const double *)(B + L.pxy) : (const double *)(B + L.xy);
    // the int ranges: a unit's flat index q ng + g, a unit id shifted by 2 bits, the padded entries <= 2 E + 64 tiles
    // (outside them build_tiles_multi runs on the host from these rows)
    const int64_t nU64 = (int64_t)Q * ng, nmax64 = std::min<int64_t>(nU64, 2 * E);
    if (d.n_scales != 2 * Q || nU64 >= (1LL << 28) || 2 * E + 64 * nmax64 >= (1LL << 31)) return refuse(gp, what, err);
    const int nU = (int)nU64, nmax = (int)nmax64;             // nmax: the units at most (every edge end flags one)
    const size_t Ez = (size_t)E, Uz = (size_t)nU, Nz = (size_t)nmax, Pz = (size_t)P;
    const int rtile = (int)((Nz + kPlanRadixTile - 1) / kPlanRadixTile);
    const int64_t scan_max = std::max<int64_t>({(int64_t)nU + 1, (int64_t)kRadixDigits * rtile, (int64_t)P + 1});
    // the scratch is an arena of its own, laid out here because it follows the group count
    size_t o = 0;
    auto piece = [&](size_t bytes) { const size_t at = o; o += pad(bytes); return at; };
    const size_t o_hdr = piece(4 * kHdrWords), o_uflag = piece(4 * Uz), o_uidx = piece(4 * (Uz + 1)), o_upt = piece(4 * Uz),
                 o_upt2 = piece(4 * Uz), o_uid = piece(4 * Uz), o_box = piece(32 * (size_t)Q), o_key0 = piece(8 * Nz), o_key1 = piece(8 * Nz),
                 o_id0 = piece(4 * Nz), o_id1 = piece(4 * Nz), o_hist = piece(4 * (size_t)kRadixDigits * rtile),
                 o_part = piece(4 * (size_t)((scan_max + kPlanScanTile - 1) / kPlanScanTile + 1)), o_cur = piece(4 * (std::max(Nz, Pz) + 1)),
                 o_urow = piece(8 * Nz), o_upair = piece(4 * (Nz + 1)), o_ustart = piece(4 * (Nz + 2)), o_egi = piece(4 * Ez),
                 o_egj = piece(4 * Ez), o_erow = piece(16 * Ez), o_ooff = piece(4 * (Nz + 1)), o_oe = piece(4 * Ez), o_okj = piece(4 * Ez),
                 o_pred = piece(4 * Ez), o_ioff = piece(4 * (Nz + 1)), o_ie = piece(4 * Ez), o_tend = piece(4 * (Nz + 1)),
                 o_ja = piece(4 * (Nz + 1)), o_jb = piece(4 * (Nz + 1)), o_mark = piece(4 * (Nz + 2)), o_midx = piece(4 * (Nz + 2)),
                 o_tstart = piece(4 * (Nz + 2)), o_tne = piece(4 * (Nz + 2)), o_tnh = piece(4 * (Nz + 2)), o_tcut = piece(4 * (Nz + 2)),
                 o_soff = piece(4 * (Pz + 1)), o_sk = piece(8 * Nz), o_spos = piece(8 * Nz);
    if (!grow(mbuf_, mcap_, o, before_alloc)) { err = "plan builder: allocation failed"; return -1; }
    if (g_timing) std::fprintf(stderr, "[deftri plan] arena of the units %.1f MiB of %.1f\n", o / 1048576.0, mcap_ / 1048576.0);
    char *M = mbuf_;
    auto ip = [&](size_t off) { return (int *)(M + off); };
    int *d_uflag = ip(o_uflag), *d_uidx = ip(o_uidx), *d_upt = ip(o_upt), *d_upt2 = ip(o_upt2), *d_uid = ip(o_uid), *d_hist = ip(o_hist),
        *d_urow = ip(o_urow), *d_upair = ip(o_upair), *d_ustart = ip(o_ustart);
    unsigned long long *d_box = (unsigned long long *)(M + o_box);
    uint64_t *d_key[2] = {(uint64_t *)(M + o_key0), (uint64_t *)(M + o_key1)};
    int *d_id[2] = {ip(o_id0), ip(o_id1)};
    TileScratch s{};
    s.hdr = ip(o_hdr); s.start = d_ustart; s.egi = ip(o_egi); s.egj = ip(o_egj); s.erow = ip(o_erow); s.ooff = ip(o_ooff); s.oe = ip(o_oe);
    s.okj = ip(o_okj); s.pred = ip(o_pred); s.ioff = ip(o_ioff); s.ie = ip(o_ie); s.tend = ip(o_tend); s.ja = ip(o_ja); s.jb = ip(o_jb);
    s.mark = ip(o_mark); s.midx = ip(o_midx); s.tstart = ip(o_tstart); s.tne = ip(o_tne); s.tnh = ip(o_tnh); s.tcut = ip(o_tcut);
    s.cur = ip(o_cur); s.part = ip(o_part); s.urow = d_urow; s.upair = d_upair;
    MultiExtras mx{};
    mx.Q = Q; mx.ng = ng; mx.D = d.n_depth; mx.dep_point = (const int *)(B + L.dep_point); mx.dscale = (const int *)(B + L.mdscale);
    mx.gp = d_gp; mx.rop = d_rop; mx.uid = d_uid; mx.uidx = d_uidx; mx.soff = ip(o_soff); mx.sk = ip(o_sk); mx.spos = ip(o_spos);

    hipEventRecord(ev_[kEvUnits], st_);
    // the units: flags and points, the pairs' boxes, the keys, the sort by (q, key, g) from ascending (q, g)
    hipMemsetAsync(s.hdr, 0, 4 * kHdrWords, st_);
    hipMemsetAsync(d_uflag, 0, 4 * Uz, st_);
    LAUNCH(k_fill, nU, (int64_t)nU, d_upt, INT_MAX);
    LAUNCH(k_fill, nU, (int64_t)nU, d_upt2, INT_MAX);
    LAUNCH(k_fill, nU, (int64_t)nU, d_uid, -1);
    LAUNCH(k_mu_flag, E, E, (const int4 *)d_ap, d_pair, d_gp, Q, ng, d_uflag, d_upt, d_upt2, s.hdr);
    hipMemcpyAsync(d_uidx, d_uflag, 4 * Uz, hipMemcpyDeviceToDevice, st_);
    hipMemsetAsync(d_uidx + nU, 0, 4, st_);
    scan(d_uidx, (int64_t)nU + 1, s.part);
    LAUNCH(k_box_init, 4 * Q, 4 * Q, d_box);
    LAUNCH(k_mu_box, nU, nU, ng, (const int *)d_uflag, (const int *)d_upt, d_pts, d_box);
    LAUNCH(k_mu_keys, nU, nU, ng, (const int *)d_uflag, (const int *)d_uidx, (const int *)d_upt, d_pts, (const unsigned long long *)d_box,
           d_key[0], d_id[0], s.hdr);
    int qbits = 0;
    while (Q >> qbits) qbits++;
    const int cur = radix_sort(d_key, d_id, d_hist, s.part, s.hdr + kHdrNu, rtile, kRadixPasses + (qbits + kPlanRadixBits - 1) / kPlanRadixBits);
    LAUNCH(k_mu_units, (int64_t)nmax + 2, nmax, ng, (const int *)d_id[cur], (const int *)d_upt, (const int *)d_upt2, d_rop, d_uid, d_urow,
           d_upair, d_ustart, (const int *)s.hdr);
    hipEventRecord(ev_[kEvUnits + 1], st_);
    hipMemcpyAsync(pin_, s.hdr, 4 * kHdrWords, hipMemcpyDeviceToHost, st_);
    hipEventRecord(ev_[kEvUnits + 2], st_);
    if (!sync(what, err)) return -1;
    static const char *const names0[] = {"dev 4a units", "dev download unit count"};
    report(kEvUnits, kEvUnits + 2, names0);
    const int *hdr = (const int *)pin_;
    if (hdr[kHdrRefuse]) return refuse(gp, what, err);
    const int32_t nu = hdr[kHdrNu];
    if (nu < 2 || nu > nmax) {
        err = "plan builder: the device wrote an impossible unit count";
        return -1;
    }
    hipEventRecord(ev_[kEvCut], st_);
    // per edge its units and rows
    LAUNCH(k_mu_edges, E, E, (const int4 *)d_ap, d_pair, d_gp, Q, ng, (const int *)d_uid, (const int *)d_upt, (const int *)d_upt2, s.egi,
           s.egj, (int4 *)s.erow, s.hdr);
    return cut_tiles(s, &mx, nu, units_max, lds_budget, before_alloc, H, order, gp, err);
}

int PlanDevice::layout(const deftri_problem_desc &d, std::function<void()> *before_alloc, SpPlanHost &H, bool download_slots,
                       int32_t &ran, std::string &err) {
    ran = 0;
    hipSetDevice(dev_);
    const Layout &L = L_;
    const int32_t P = P_, S = d.n_scales;
    const int64_t E = E_, D = d.n_depth, nloc = (int64_t)H.arap_ids.size();
    const int32_t nao = H.n_arap_owned;
    if (!buf_ || !on_.layout || nloc_ < 0 || nloc_ != nloc || P != d.n_points || E != d.n_arap ||
        (on_.multi ? d.n_pairs < 2 : d.n_pairs != 1 || S > 2) || S < 0 || nao < 0 || nao > nloc || (int64_t)H.dep_ids.size() != D || (D > 0 && S < 1) || H.lo != 0 || H.hi != P || P < 1) {
        err = "plan builder: layout() without the edges of this problem";
        return -1;
    }
    // several pairs (on_.multi): stage 7 is written for one pair and two scales, so it stays on the host
    const bool dev7 = !on_.multi;
    int n0 = 0;                                           // depth edges of scale 0
    for (int64_t e = 0; dev7 && e < D; e++) n0 += d.dep_scale[e] == 0;
    auto blocks = [](int64_t n) { return (n + kSpBlock - 1) / kSpBlock; };
    const int64_t nb = dev7 ? blocks(nao) + blocks(nloc - nao) + blocks(n0) + blocks(D - n0) : 0;
    const int ni = (P + 31) / 32, nwin = (P + kSpSortWindow - 1) / kSpSortWindow;
    if (dev7 && nb > E / kSpBlock + D / kSpBlock + 4) { err = "plan builder: more phase-1 blocks than the arena holds"; return -1; }
    // the wave layout's int scan: a row holds at most 2 kPlanRunMax slots, a wave's steps are one row's count
    const bool waves = 16 * (int64_t)P < (1LL << 31);
    char *B = buf_;
    const int *d_ap = (const int *)(B + L.ap), *d_rop = (const int *)(B + L.rop), *d_aid = (const int *)(B + L.aid),
              *d_dep_point = (const int *)(B + L.dep_point), *d_dep_ids = (const int *)(B + L.dep_ids),
              *d_dep_off = (const int *)(B + L.dep_off), *d_ioff = (const int *)(B + L.ioff), *d_inc = (const int *)(B + L.inc);
    const int *d_dscale = (const int *)(B + L.dscale);       // uploaded by rows() with the other inputs
    int *d_dflag = (int *)(B + L.dflag), *d_bkey = (int *)(B + L.bkey), *d_boff = (int *)(B + L.boff),
        *d_bord = (int *)(B + L.bord), *d_order = (int *)(B + L.order), *d_scnt = (int *)(B + L.scnt), *d_wnext = (int *)(B + L.wnext),
        *d_wsteps = (int *)(B + L.wsteps), *d_wsp = (int *)(B + L.wsp), *d_wja = (int *)(B + L.wja), *d_wjb = (int *)(B + L.wjb),
        *d_wmark = (int *)(B + L.wmark), *d_widx = (int *)(B + L.widx), *d_wsoff = (int *)(B + L.wsoff), *d_hdr = (int *)(B + L.lhdr),
        *d_dperm = (int *)(B + L.dperm), *d_hvb = (int *)(B + L.hvb), *d_hvoff = (int *)(B + L.hvoff), *d_rowmap = (int *)(B + L.rowmap),
        *d_woff = (int *)(B + L.woff);
    int4 *d_blk0 = (int4 *)(B + L.blk0), *d_blk = (int4 *)(B + L.blk);
    uint8_t *d_wsplit = (uint8_t *)(B + L.wsplit);

    hipEventRecord(ev_[kEvLayout], st_);
    // 7. dperm, the blocks, their dispatch order, the heavy vertices' lists
    hipMemsetAsync(d_hdr, 0, 4 * kHdrWords, st_);
    hipMemsetAsync(d_hvoff, 0, 4 * 4, st_);
    if (dev7) {
        LAUNCH(k_dep_flag, D + 1, (int)D, d_dep_ids, d_dscale, d_dflag);
        scan(d_dflag, D + 1);
        LAUNCH(k_dperm, D, (int)D, d_dep_ids, d_dscale, (const int *)d_dflag, d_dperm);
        LAUNCH(k_blk_make, nb, (int)nb, (int)nao, (int)nloc, n0, (int)D, d_aid, d_ap, d_rop, d_dep_point, d_dep_ids,
               (const int *)d_dperm, d_dscale, d_blk0, d_bkey);
        sort_by_row(nb, d_bkey, P, d_boff, d_bord, d_hdr);
        LAUNCH(k_blk_deal, nb, (int)nb, (const int *)d_bord, (const int4 *)d_blk0, d_blk);
        hipLaunchKernelGGL(dev::k_blk_heavy, dim3(1), dim3(1024), 0, st_, (int)nb, 1 + S, (const int4 *)d_blk, d_hvb, d_hvoff);
    }
    hipEventRecord(ev_[kEvLayout + 1], st_);
    // 8b. the windows' rows by slot count, the wave cut from every multiple of 32, the chain from row 0
    if (waves) {
        const int64_t nodes = (int64_t)ni + 1;
        hipLaunchKernelGGL(dev::k_win_sort, dim3((unsigned)std::min(nwin, kGridMax)), dim3(kSpSortWindow), 0, st_, P, nwin, d_ioff,
                           d_dep_off, d_order, d_scnt);
        LAUNCH(k_wave_cut, nodes, P, ni, (const int *)d_scnt, d_wnext, d_wsteps, d_wsp);
        hipMemsetAsync(d_wmark, 0, 4 * (size_t)nodes, st_);
        LAUNCH(k_fill, 1, (int64_t)1, d_wmark, 1);
        int rounds = 1;
        while (((int64_t)1 << (rounds - 1)) < nodes) rounds++;
        const int *jin = d_wnext;
        int *jout = d_wja;
        for (int r = 0; r < rounds; r++) {
            LAUNCH(k_tile_jump, nodes, nodes, jin, jout, d_wmark, (const int *)d_hdr);
            jin = jout;
            jout = jout == d_wja ? d_wjb : d_wja;
        }
        LAUNCH(k_wave_marks, nodes, ni, (const int *)d_wmark, (const int *)d_wsteps, d_widx, d_wsoff);
        scan(d_widx, nodes);
        scan(d_wsoff, nodes);
        LAUNCH(k_wave_write, 64 * (int64_t)ni, P, ni, (const int *)d_wmark, (const int *)d_widx, (const int *)d_wsoff, (const int *)d_wsp,
               (const int *)d_order, d_rowmap, d_woff, d_wsplit, d_hdr);
    }
    hipEventRecord(ev_[kEvLayout + 2], st_);
    hipMemcpyAsync(pin_, B + L.dl3, (waves ? L.dl3_end : L.rowmap) - L.dl3, hipMemcpyDeviceToHost, st_);
    hipEventRecord(ev_[kEvLayout + 3], st_);
    if (!sync("layout", err)) return -1;
    static const char *const names1[] = {"dev 7 phase-1 blocks", "dev 8b row sort, wave cut", "dev download layout"};
    report(kEvLayout, kEvLayout + 3, names1);
    const int *hdr = (const int *)(pin_ + (L.lhdr - L.dl3)), *hvoff = (const int *)(pin_ + (L.hvoff - L.dl3));
    if (hdr[kHdrBound]) return 1;
    const int32_t nw = waves ? hdr[kLhNw] : 0;
    const int64_t nsl = waves ? hdr[kLhSlots] : 0;
    if ((dev7 && (hvoff[0] != 0 || hvoff[1 + S] < 0 || hvoff[1 + S] > nb)) || (waves && (nw < 1 || nw > ni || nsl < 0 || nsl > 16 * (int64_t)P))) {
        err = "plan builder: the device wrote impossible layout counts";
        return -1;
    }
    auto t0 = std::chrono::steady_clock::now();
    if (dev7) {
        take(H.dperm, pin_, L.dperm - L.dl3, (size_t)D);
        take(H.blk, pin_, L.blk - L.dl3, 4 * (size_t)nb);
        take(H.hv_blk, pin_, L.hvb - L.dl3, (size_t)hvoff[1 + S]);
        H.hv_blk_off.assign(hvoff, hvoff + 1 + S + 1);
        ran |= 1;
    }
    // (the host builds stage 8b when 64 x slots does not fit an int)
    if (!waves || 64 * nsl >= (1LL << 31)) return 0;
    take(H.rowmap, pin_, L.rowmap - L.dl3, 64 * (size_t)nw);
    take(H.wsplit, pin_, L.wsplit - L.dl3, (size_t)nw);
    {
        const int *wo = (const int *)(pin_ + (L.woff - L.dl3));
        H.woff.assign(wo, wo + nw + 1);
    }
    if (g_timing) std::fprintf(stderr, "[deftri plan] %-28s %8.2f ms\n", "dev staging -> layout arrays", ms_since(t0));
    // the slot arrays: pmap | pidx in a buffer of their own, kept for the solver's device-to-device copy
    const size_t nel = 64 * (size_t)nsl, half = pad(4 * nel), need = 2 * half;
    if (!grow(sbuf_, scap_, need, before_alloc)) { err = "plan builder: allocation failed"; return -1; }
    int *d_pmap = (int *)sbuf_, *d_pidx = (int *)(sbuf_ + half);
    hipEventRecord(ev_[kEvSlots], st_);
    if (nel > 0) {
        hipMemsetAsync(sbuf_, 0xff, need, st_);
        LAUNCH(k_slot_fill, 64 * (int64_t)nw, nw, (int)nsl, (const int *)d_rowmap, (const int *)d_woff, (const uint8_t *)d_wsplit, d_ioff,
               d_inc, d_dep_off, d_dep_ids, d_dscale, d_pmap, d_pidx, d_hdr);
    }
    hipEventRecord(ev_[kEvSlots + 1], st_);
    hipMemcpyAsync(pin_, d_hdr, 4 * kHdrWords, hipMemcpyDeviceToHost, st_);
    if (download_slots && nel > 0) {
        H.pmap.resize(nel);
        H.pidx.resize(nel);
        hipMemcpyAsync(H.pmap.data(), d_pmap, 4 * nel, hipMemcpyDeviceToHost, st_);
        hipMemcpyAsync(H.pidx.data(), d_pidx, 4 * nel, hipMemcpyDeviceToHost, st_);
    }
    hipEventRecord(ev_[kEvSlots + 2], st_);
    if (!sync("layout", err)) return -1;
    static const char *const names2[] = {"dev 8b slot fill", "dev download slots"};
    report(kEvSlots, kEvSlots + 2, names2);
    if (((const int *)pin_)[kHdrBound]) return 1;
    H.pmap_dev = nel > 0 ? d_pmap : nullptr;
    H.pidx_dev = nel > 0 ? d_pidx : nullptr;
    H.slots_dev = (int64_t)nel;
    ran |= 6;
    return 0;
}

}  // namespace deftri
