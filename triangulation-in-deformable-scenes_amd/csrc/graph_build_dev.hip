// graph_build_dev.hip — the full ARAP graph build on the device (deftri_set_graph_builder(1)): what
// build_arap_graph's host passes do after the triangulation, stage by stage (the bits of deftri_graph_build_info):
//   0 CSR adjacency   two candidate entries per triangle corner, scan, fill, per-row bounded sort + unique, scan, compaction
//   1 vector map      createVectorMap over a 1-D bucket grid on x; inv by an atomic maximum
//   2 geometry        graph_dev.hip's k_cot_corners / k_cot_finish / k_compute_r on the resident arrays
//   3 slot scan       scan_pair's filters per slot, the first-encounter order by a 64-bit atomic minimum
//   4 point numbering each id's first occurrence by an atomic minimum over the direct id table, flagged and scanned
//   5 edges           emit_pair_edges per slot at the scanned offsets
// Every output is a function of its inputs alone (sorted rows, minima, maxima, scans), so the arrays are the host's.
// Every size the host needs comes down in one small download; one download through pinned staging brings the arrays.
// Built with -ffp-contract=off: the isApprox test and rep_info round as the host's expressions do.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "graph_builder.h"

namespace deftri {

namespace {
constexpr int kB = 256;
constexpr int kScanItems = 4;
constexpr int kScanTile = kB * kScanItems;
constexpr int kRowBound = 64;      // candidate entries of one CSR row (twice its triangles): longer rows go to the host
constexpr int kSortBlock = 64;

constexpr int kFlagInput = 1;      // an input error: the host build reports it
constexpr int kFlagRow = 2;        // a row longer than kRowBound
constexpr int kFlagIndex = 4;      // a triangle index or a MapPoint id outside its table

struct DKf {
    const int64_t *pid;
    const float *pos, *uv, *depth, *isig;
    const int32_t *obs, *oct;
    const double *meas;
    const uint8_t *status;
    int n_slots, n_obs, n_scales;
};

struct DPair {
    int a, b, q, ns12, n1, n2, c1, c2, s1, s2, rot_base;
    int64_t sbase, wpad;           // the pair's first slot in the concatenated per-slot arrays; its weights in the padded w
    const int32_t *off, *adj, *pos_idx, *inv;
};

__global__ __launch_bounds__(kB) void k_fill_i32(int32_t *__restrict__ p, int64_t n, int32_t v) {
    const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ __launch_bounds__(kB) void k_fill_u64(unsigned long long *__restrict__ p, int64_t n, unsigned long long v) {
    const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- exclusive scan of n int32 into out[0..n] (out[n] the total): tiles, the tile sums in one block, the add ----
__device__ __forceinline__ int32_t block_scan_inclusive(int32_t *sh, int32_t v) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < kB; d <<= 1) {
        const int32_t t = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    return sh[tid];
}

__global__ __launch_bounds__(kB) void k_scan_tiles(const int32_t *__restrict__ in, int32_t *__restrict__ out, int64_t n,
                                                   int32_t *__restrict__ bsum) {
    __shared__ int32_t sh[kB];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int32_t v[kScanItems], s = 0;
    for (int k = 0; k < kScanItems; k++) {
        v[k] = base + k < n ? in[base + k] : 0;
        s += v[k];
    }
    const int32_t incl = block_scan_inclusive(sh, s);
    int32_t excl = incl - s;
    for (int k = 0; k < kScanItems; k++) {
        if (base + k < n) out[base + k] = excl;
        excl += v[k];
    }
    if (threadIdx.x == kB - 1) bsum[blockIdx.x] = incl;
}

__global__ __launch_bounds__(kB) void k_scan_sums(int32_t *__restrict__ bsum, int nb) {
    __shared__ int32_t sh[kB];
    __shared__ int32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int c = 0; c < nb; c += kB) {
        const int i = c + threadIdx.x;
        const int32_t v = i < nb ? bsum[i] : 0;
        const int32_t incl = block_scan_inclusive(sh, v);
        const int32_t c0 = carry;
        __syncthreads();
        if (i < nb) bsum[i] = incl - v + c0;
        if (threadIdx.x == kB - 1) carry = c0 + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(kB) void k_scan_add(int32_t *__restrict__ out, int64_t n, const int32_t *__restrict__ bsum, int nb) {
    const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (i < n) out[i] += bsum[i / kScanTile];
    else if (i == n) out[n] = bsum[nb];
}

// ---- stage 0: CSR adjacency ----
__global__ __launch_bounds__(kB) void k_adj_count(int ntri, const int32_t *__restrict__ tris, int n1, int32_t *__restrict__ cnt,
                                                  int *__restrict__ flags) {
    const int64_t c = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (c >= 3 * (int64_t)ntri) return;
    const int v = tris[c];
    if ((unsigned)v >= (unsigned)n1) { atomicOr(flags, kFlagIndex); return; }
    atomicAdd(cnt + v, 2);
}

__global__ __launch_bounds__(kB) void k_adj_fill(int ntri, const int32_t *__restrict__ tris, int n1, const int32_t *__restrict__ coff,
                                                 int32_t *__restrict__ cur, int32_t *__restrict__ tmp, int64_t cap) {
    const int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (t >= ntri) return;
    const int v[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
    for (int k = 0; k < 3; k++)
        if ((unsigned)v[k] >= (unsigned)n1) return;                      // flagged by k_adj_count
    for (int k = 0; k < 3; k++) {
        const int64_t at = (int64_t)coff[v[k]] + atomicAdd(cur + v[k], 2);
        if (at < 0 || at + 1 >= cap) continue;
        tmp[at] = v[(k + 1) % 3];
        tmp[at + 1] = v[(k + 2) % 3];
    }
}

// one thread per row: an insertion sort of at most kRowBound entries in LDS (column tid), unique, written back in place
__global__ __launch_bounds__(kSortBlock) void k_adj_sort(int n1, const int32_t *__restrict__ coff, int32_t *__restrict__ tmp,
                                                         int32_t *__restrict__ ucnt, int *__restrict__ flags) {
    __shared__ int32_t row[kRowBound * kSortBlock];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kSortBlock + tid;
    if (i >= n1) return;
    const int32_t b = coff[i];
    const int len = coff[i + 1] - b;
    if (len < 0 || len > kRowBound) { atomicOr(flags, kFlagRow); ucnt[i] = 0; return; }
    for (int r = 0; r < len; r++) {
        const int32_t v = tmp[b + r];
        int j = r;
        while (j > 0 && row[(j - 1) * kSortBlock + tid] > v) { row[j * kSortBlock + tid] = row[(j - 1) * kSortBlock + tid]; j--; }
        row[j * kSortBlock + tid] = v;
    }
    int u = 0;
    int32_t prev = -1;
    for (int r = 0; r < len; r++) {
        const int32_t v = row[r * kSortBlock + tid];
        if (r == 0 || v != prev) { tmp[b + u] = v; u++; prev = v; }
    }
    ucnt[i] = u;
}

__global__ __launch_bounds__(kB) void k_adj_compact(int n1, const int32_t *__restrict__ coff, const int32_t *__restrict__ off,
                                                    const int32_t *__restrict__ tmp, int32_t *__restrict__ adj, int64_t cap) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n1) return;
    const int64_t src = coff[i], dst = off[i];
    int len = off[i + 1] - off[i];
    if (len > kRowBound) len = kRowBound;
    for (int r = 0; r < len; r++)
        if (dst + r < cap && src + r < cap) adj[dst + r] = tmp[src + r];
}

// ---- stage 1: vector map ----
__device__ __forceinline__ int bucket_of(double x, double xmin, double inv_h, int nb) {
    const double t = (x - xmin) * inv_h;
    return t > 0 ? (t < (double)nb ? (int)t : nb - 1) : 0;
}

__global__ __launch_bounds__(kB) void k_bucket_count(int n1, const double *__restrict__ pos, double xmin, double inv_h, int nb,
                                                     int32_t *__restrict__ bcnt) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n1) return;
    atomicAdd(bcnt + bucket_of(pos[3 * (int64_t)i], xmin, inv_h, nb), 1);
}

__global__ __launch_bounds__(kB) void k_bucket_fill(int n1, const double *__restrict__ pos, double xmin, double inv_h, int nb,
                                                    const int32_t *__restrict__ boff, int32_t *__restrict__ bcur,
                                                    int32_t *__restrict__ items) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= n1) return;
    const int b = bucket_of(pos[3 * (int64_t)i], xmin, inv_h, nb);
    const int64_t at = (int64_t)boff[b] + atomicAdd(bcur + b, 1);
    if (at >= 0 && at < n1) items[at] = i;
}

// pos_idx[k]: the smallest p < k in the host's x window (|x_p - x_k| <= sqrt(1e-12 |v_k|^2)) that passes isApprox, else k.
// The buckets searched cover the window with a margin; the window test itself is the host's.
__global__ __launch_bounds__(kB) void k_vector_map(int n1, const double *__restrict__ pos, double xmin, double inv_h, int nb,
                                                   const int32_t *__restrict__ boff, const int32_t *__restrict__ items,
                                                   int32_t *__restrict__ pos_idx, int *__restrict__ nonident) {
    const int k = blockIdx.x * kB + threadIdx.x;
    if (k >= n1) return;
    const double *v = pos + 3 * (int64_t)k;
    const double prec2 = 1e-12;
    const double nk = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const double rad = sqrt(prec2 * nk);
    int best = k;
    int b0 = bucket_of(v[0] - 1.001 * rad, xmin, inv_h, nb) - 1, b1 = bucket_of(v[0] + 1.001 * rad, xmin, inv_h, nb) + 1;
    if (!(rad == rad) || rad > 1.7e308) { b0 = 0; b1 = nb - 1; }
    b0 = max(b0, 0);
    b1 = min(b1, nb - 1);
    const int t1 = min(boff[b1 + 1], n1);
    for (int t = max(boff[b0], 0); t < t1; t++) {
        const int p = items[t];
        if (p >= best || p < 0) continue;
        const double *w = pos + 3 * (int64_t)p;
        if (fabs(w[0] - v[0]) > rad) continue;
        const double dx = v[0] - w[0], dy = v[1] - w[1], dz = v[2] - w[2];
        const double np = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
        if (dx * dx + dy * dy + dz * dz <= prec2 * fmin(nk, np)) best = p;
    }
    pos_idx[k] = best;
    if (best != k) atomicOr(nonident, 1);
}

__global__ __launch_bounds__(kB) void k_inverse_map(int n1, const int32_t *__restrict__ pos_idx, int32_t *__restrict__ inv) {
    const int v = blockIdx.x * kB + threadIdx.x;
    if (v >= n1) return;
    const int p = pos_idx[v];
    if ((unsigned)p < (unsigned)n1) atomicMax(inv + p, v);
}

// ---- stage 3: slot scan ----
// scan_pair's filters for slot mp; true: the slot emits its observation (and then its ARAP neighbours)
__device__ __forceinline__ bool slot_emits(const DKf &kf1, const DKf &kf2, int mp, bool &both, int32_t &o1, int32_t &o2,
                                           int *__restrict__ flags) {
    both = kf1.pid[mp] >= 0 && kf2.pid[mp] >= 0;
    if (!both) return false;
    o1 = kf1.obs[mp];
    o2 = kf2.obs[mp];
    if (o1 < 0 || o2 < 0) return false;
    if (o1 >= kf1.n_obs || o2 >= kf2.n_obs) { if (flags) atomicOr(flags, kFlagInput); return false; }
    const int32_t oc1 = kf1.oct[o1], oc2 = kf2.oct[o2];
    if (oc1 < 0 || oc1 >= kf1.n_scales || oc2 < 0 || oc2 >= kf2.n_scales) { if (flags) atomicOr(flags, kFlagInput); return false; }
    if ((kf1.status && kf1.status[o1]) || (kf2.status && kf2.status[o2])) { if (flags) atomicOr(flags, kFlagInput); return false; }
    return true;
}

// the neighbour slot of CSR entry k, or -1 where emit_pair_edges' filter drops it
__device__ __forceinline__ int neighbour_slot(const DKf &kf1, const DKf &kf2, const DPair &P, int32_t k) {
    const int j = P.adj[k];
    if ((unsigned)j >= (unsigned)P.n1) return -1;
    const int slot = P.pos_idx[j];
    if (slot < 0 || slot >= P.ns12 || kf1.pid[slot] < 0 || kf2.pid[slot] < 0) return -1;
    return slot;
}

// the row of slot mp (its vertex i and CSR range), false where the slot has no ARAP edges
__device__ __forceinline__ bool slot_row(const DPair &P, int mp, int &i, int32_t &k0, int32_t &k1) {
    if (mp >= P.n1) return false;
    i = P.inv[mp];
    if (i < 0 || i >= P.n1) return false;
    k0 = P.off[i];
    k1 = min(P.off[i + 1], k0 + kRowBound);
    return true;
}

__device__ __forceinline__ unsigned long long enc_key(int mp, int local) {
    return ((unsigned long long)(unsigned)mp << 32) | (unsigned)local;
}

__global__ __launch_bounds__(kB) void k_slot_scan(DKf kf1, DKf kf2, DPair P, unsigned long long *__restrict__ key,
                                                  int32_t *__restrict__ cobs, int32_t *__restrict__ carap, int *__restrict__ flags) {
    const int mp = blockIdx.x * kB + threadIdx.x;
    if (mp >= P.ns12) return;
    bool both;
    int32_t o1, o2;
    int nar = 0;
    const bool emits = slot_emits(kf1, kf2, mp, both, o1, o2, flags);
    if (both) atomicMin(key + P.sbase + mp, enc_key(mp, 0));
    int i;
    int32_t k0, k1;
    if (emits && slot_row(P, mp, i, k0, k1))
        for (int32_t k = k0; k < k1; k++) {
            const int slot = neighbour_slot(kf1, kf2, P, k);
            if (slot < 0) continue;
            atomicMin(key + P.sbase + slot, enc_key(mp, 1 + k - k0));
            nar++;
        }
    cobs[P.sbase + mp] = emits ? 1 : 0;
    carap[P.sbase + mp] = nar;
}

// pass 0 counts the slots whose key is one of mp's candidate keys, pass 1 writes them at the scanned offset
template <bool WRITE>
__global__ __launch_bounds__(kB) void k_enc(DKf kf1, DKf kf2, DPair P, const unsigned long long *__restrict__ key,
                                            int32_t *__restrict__ cenc, const int32_t *__restrict__ senc,
                                            int32_t *__restrict__ enc, int32_t *__restrict__ encq, int64_t cap) {
    const int mp = blockIdx.x * kB + threadIdx.x;
    if (mp >= P.ns12) return;
    bool both;
    int32_t o1, o2;
    const bool emits = slot_emits(kf1, kf2, mp, both, o1, o2, nullptr);
    int n = 0;
    int64_t at = WRITE ? senc[P.sbase + mp] : 0;
    if (both && key[P.sbase + mp] == enc_key(mp, 0)) {
        if (WRITE && at >= 0 && at < cap) { enc[at] = mp; encq[at] = P.q; at++; }
        n++;
    }
    int i;
    int32_t k0, k1;
    if (emits && slot_row(P, mp, i, k0, k1))
        for (int32_t k = k0; k < k1; k++) {
            const int slot = neighbour_slot(kf1, kf2, P, k);
            if (slot < 0 || key[P.sbase + slot] != enc_key(mp, 1 + k - k0)) continue;
            if (WRITE && at >= 0 && at < cap) { enc[at] = slot; encq[at] = P.q; at++; }
            n++;
        }
    if (!WRITE) cenc[P.sbase + mp] = n;
}

// ---- stage 4: point numbering ----
// occurrence j = 2 (index in enc, the pairs concatenated) + side; side 0 is the pair's keyframe 1
__device__ __forceinline__ bool occurrence(int64_t j, const int32_t *__restrict__ senc_total, const int32_t *__restrict__ enc,
                                           const int32_t *__restrict__ encq, const DPair *__restrict__ pairs, int npairs,
                                           const DKf *__restrict__ kfs, int64_t lo, int64_t span, int &q, int &kf, int &slot,
                                           int64_t &idx) {
    if (j >= 2 * (int64_t)senc_total[0]) return false;
    q = encq[j >> 1];
    slot = enc[j >> 1];
    if ((unsigned)q >= (unsigned)npairs) return false;
    kf = (j & 1) ? pairs[q].a : pairs[q].b;
    if (slot < 0 || slot >= kfs[kf].n_slots) return false;
    idx = kfs[kf].pid[slot] - lo;
    return idx >= 0 && idx < span;
}

__global__ __launch_bounds__(kB) void k_occ_first(int64_t cap, const int32_t *__restrict__ senc_total, const int32_t *__restrict__ enc,
                                                  const int32_t *__restrict__ encq, const DPair *__restrict__ pairs, int npairs,
                                                  const DKf *__restrict__ kfs, int64_t lo, int64_t span, int32_t *__restrict__ first,
                                                  int *__restrict__ flags) {
    const int64_t j = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (j >= cap) return;
    int q, kf, slot;
    int64_t idx;
    if (!occurrence(j, senc_total, enc, encq, pairs, npairs, kfs, lo, span, q, kf, slot, idx)) {
        if (j < 2 * (int64_t)senc_total[0]) atomicOr(flags, kFlagIndex);
        return;
    }
    atomicMin(first + idx, (int32_t)j);
}

__global__ __launch_bounds__(kB) void k_occ_flag(int64_t cap, const int32_t *__restrict__ senc_total, const int32_t *__restrict__ enc,
                                                 const int32_t *__restrict__ encq, const DPair *__restrict__ pairs, int npairs,
                                                 const DKf *__restrict__ kfs, int64_t lo, int64_t span,
                                                 const int32_t *__restrict__ first, int32_t *__restrict__ isfirst) {
    const int64_t j = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (j >= cap) return;
    int q, kf, slot;
    int64_t idx;
    const bool ok = occurrence(j, senc_total, enc, encq, pairs, npairs, kfs, lo, span, q, kf, slot, idx);
    isfirst[j] = ok && first[idx] == (int32_t)j ? 1 : 0;
}

__global__ __launch_bounds__(kB) void k_occ_write(int64_t cap, const int32_t *__restrict__ senc_total, const int32_t *__restrict__ enc,
                                                  const int32_t *__restrict__ encq, const DPair *__restrict__ pairs, int npairs,
                                                  const DKf *__restrict__ kfs, int64_t lo, int64_t span,
                                                  const int32_t *__restrict__ first, const int32_t *__restrict__ pnum,
                                                  int64_t *__restrict__ point_mpid, double *__restrict__ points,
                                                  float *__restrict__ point_orig, double *__restrict__ order_xy,
                                                  int32_t *__restrict__ point_kf, int32_t *__restrict__ point_slot,
                                                  int32_t *__restrict__ order_kf, int32_t *__restrict__ order_slot,
                                                  int32_t *__restrict__ slot_pt) {
    const int64_t j = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (j >= cap) return;
    int q, kf, slot;
    int64_t idx;
    if (!occurrence(j, senc_total, enc, encq, pairs, npairs, kfs, lo, span, q, kf, slot, idx)) return;
    const int32_t f = first[idx];
    if (f < 0 || f >= cap) return;
    const int64_t k = pnum[f];
    if (k < 0 || k >= cap) return;
    if (slot < pairs[q].ns12) slot_pt[2 * (pairs[q].sbase + slot) + (j & 1)] = (int32_t)k;
    if (f != (int32_t)j) return;
    const int okf = pairs[q].b;
    point_mpid[k] = kfs[kf].pid[slot];
    const float *p = kfs[kf].pos + 3 * (int64_t)slot;
    for (int c = 0; c < 3; c++) { points[3 * k + c] = (double)p[c]; point_orig[3 * k + c] = p[c]; }
    const float *o = kfs[okf].pos + 3 * (int64_t)slot;          // slot < ns12 <= the ordering keyframe's slots
    order_xy[2 * k] = (double)o[0];
    order_xy[2 * k + 1] = (double)o[1];
    point_kf[k] = kf; point_slot[k] = slot;
    order_kf[k] = okf; order_slot[k] = slot;
}

// ---- stage 5: edges ----
struct EdgeOut {
    int32_t *rep_point, *rep_cam, *dep_point, *dep_scale, *dep_cam, *arap_pts, *arap_pair, *arap_rot;
    double *rep_obs, *rep_base, *rep_info, *dep_meas, *dep_info, *arap_w;
    int64_t *arap_wk;
    int64_t cap_obs, cap_arap;     // edges of each kind the arrays hold
};

__global__ __launch_bounds__(kB) void k_edges(DKf kf1, DKf kf2, DPair P, const int32_t *__restrict__ sobs,
                                              const int32_t *__restrict__ sarap, const int32_t *__restrict__ slot_pt,
                                              const double *__restrict__ wpad, const int64_t *__restrict__ woff, double rep_weight,
                                              double info_dep, EdgeOut g) {
    const int mp = blockIdx.x * kB + threadIdx.x;
    if (mp >= P.ns12) return;
    bool both;
    int32_t o1, o2;
    if (!slot_emits(kf1, kf2, mp, both, o1, o2, nullptr)) return;
    const int64_t r = 2 * (int64_t)sobs[P.sbase + mp];
    if (r < 0 || r + 1 >= 2 * g.cap_obs) return;
    const int32_t p1 = slot_pt[2 * (P.sbase + mp)], p2 = slot_pt[2 * (P.sbase + mp) + 1];
    const double base1 = (double)kf1.isig[kf1.oct[o1]], base2 = (double)kf2.isig[kf2.oct[o2]];
    g.rep_point[r] = p1; g.rep_cam[r] = P.c1;
    g.rep_obs[2 * r] = (double)kf1.uv[2 * (int64_t)o1]; g.rep_obs[2 * r + 1] = (double)kf1.uv[2 * (int64_t)o1 + 1];
    g.rep_base[r] = base1; g.rep_info[r] = base1 * rep_weight;
    g.rep_point[r + 1] = p2; g.rep_cam[r + 1] = P.c2;
    g.rep_obs[2 * r + 2] = (double)kf2.uv[2 * (int64_t)o2]; g.rep_obs[2 * r + 3] = (double)kf2.uv[2 * (int64_t)o2 + 1];
    g.rep_base[r + 1] = base2; g.rep_info[r + 1] = base2 * rep_weight;
    g.dep_point[r] = p1; g.dep_scale[r] = P.s1; g.dep_cam[r] = P.c1;
    g.dep_meas[r] = kf1.meas ? kf1.meas[o1] : (double)kf1.depth[o1]; g.dep_info[r] = info_dep;
    g.dep_point[r + 1] = p2; g.dep_scale[r + 1] = P.s2; g.dep_cam[r + 1] = P.c2;
    g.dep_meas[r + 1] = kf2.meas ? kf2.meas[o2] : (double)kf2.depth[o2]; g.dep_info[r + 1] = info_dep;
    int i;
    int32_t k0, k1;
    if (!slot_row(P, mp, i, k0, k1)) return;
    int64_t e = sarap[P.sbase + mp];
    const int64_t w0 = woff[P.q];
    for (int32_t k = k0; k < k1; k++) {
        const int slot = neighbour_slot(kf1, kf2, P, k);
        if (slot < 0) continue;
        if (e < 0 || e >= g.cap_arap) return;
        g.arap_pts[4 * e] = p1; g.arap_pts[4 * e + 1] = p2;
        g.arap_pts[4 * e + 2] = slot_pt[2 * (P.sbase + slot)]; g.arap_pts[4 * e + 3] = slot_pt[2 * (P.sbase + slot) + 1];
        g.arap_pair[e] = P.q;
        g.arap_rot[2 * e] = P.rot_base + i; g.arap_rot[2 * e + 1] = P.rot_base + P.adj[k];
        g.arap_w[e] = wpad[P.wpad + k];
        g.arap_wk[e] = w0 + k;
        e++;
    }
}

// every pair's offset in the concatenated weights (the sum of the earlier pairs' CSR sizes)
__global__ void k_pair_offsets(const DPair *__restrict__ pairs, int npairs, int64_t *__restrict__ woff) {
    if (blockIdx.x || threadIdx.x) return;
    int64_t acc = 0;
    for (int q = 0; q < npairs; q++) {
        woff[q] = acc;
        acc += pairs[q].off[pairs[q].n1];
    }
}

// the sizes the host needs: ctl[4] occurrences / 2, [5] observations, [6] ARAP edges, [7] points
__global__ void k_counts(const int32_t *__restrict__ senc_total, const int32_t *__restrict__ sobs_total,
                         const int32_t *__restrict__ sarap_total, const int32_t *__restrict__ pnum_total, int32_t *__restrict__ ctl) {
    if (blockIdx.x || threadIdx.x) return;
    ctl[4] = senc_total[0];
    ctl[5] = sobs_total[0];
    ctl[6] = sarap_total[0];
    ctl[7] = pnum_total[0];
}

__global__ void k_mesh_count(const int32_t *__restrict__ off, int n1, int32_t *__restrict__ dst) {
    if (blockIdx.x || threadIdx.x) return;
    dst[0] = off[n1];
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct Bump {
    char *base = nullptr;
    size_t at = 0;
    template <class T>
    T *take(size_t n) {
        T *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += align_up(sizeof(T) * std::max<size_t>(n, 1));
        return p;
    }
};

unsigned grid(int64_t n, int block = kB) { return (unsigned)std::max<int64_t>(1, (n + block - 1) / block); }
}  // namespace

GraphBuilderDevice::GraphBuilderDevice(int device, hipStream_t st) : dev_(device), st_(st) {}

GraphBuilderDevice::~GraphBuilderDevice() {
    hipSetDevice(dev_);
    if (buf_ || pin_) hipStreamSynchronize(st_);
    if (buf_) hipFree(buf_);
    if (pin_) hipHostFree(pin_);
    for (hipEvent_t e : ev_)
        if (e) hipEventDestroy(e);
}

int GraphBuilderDevice::build(const deftri_map &map, const std::vector<DepthView> &dv, std::vector<MeshIn> &meshes,
                              const std::vector<PairIn> &pairs, int64_t id_lo, int64_t span, double rep_weight, double info_dep,
                              GraphResult &g, int &reason, std::string &err) {
    hipSetDevice(dev_);
    reason = 0;
    bytes_up = bytes_down = 0;
    syncs = 0;
    for (double &s : stage_ms) s = 0;
    bool ok = true;
    auto check = [&](hipError_t e, const char *what) {
        if (e != hipSuccess && ok) {
            err = std::string("graph build on the device: ") + what + ": " + hipGetErrorString(e);
            ok = false;
        }
        return e == hipSuccess;
    };
    const int K = map.n_keyframes, NM = (int)meshes.size(), NP = (int)pairs.size();
    // what of the map the pairs read
    std::vector<char> used((size_t)K, 0);
    for (const PairIn &p : pairs) used[p.a] = used[p.b] = 1;
    int64_t S = 0, n1sum = 0, wsum = 0;
    std::vector<int64_t> sbase(NP), wpad(NP);
    for (int q = 0; q < NP; q++) {
        sbase[q] = S;
        S += pairs[q].ns12;
        wpad[q] = wsum;
        wsum += 6 * (int64_t)meshes[pairs[q].mesh].ntri;
        n1sum += meshes[pairs[q].mesh].n1;
    }
    const int64_t cap_occ = 2 * S, cap_obs = S, cap_arap = wsum;   // upper bounds of the counts (the caller checked int32)
    int64_t scan_max = std::max<int64_t>(cap_occ, 1);
    for (const MeshIn &m : meshes) scan_max = std::max<int64_t>(scan_max, (int64_t)m.n1 + 1);

    struct DMesh {
        double *pos;
        int32_t *tris, *cnt, *coff, *cur, *tmp, *ucnt, *off, *adj, *pos_idx, *inv, *bcnt, *boff, *bcur, *items;
    };
    struct DKfBuf {
        int64_t *pid;
        float *pos, *uv, *depth, *isig;
        int32_t *obs, *oct;
        double *meas;
        uint8_t *status;
    };
    std::vector<DMesh> dm(NM);
    std::vector<DKfBuf> dk(K);
    std::vector<double *> dpos2(NP);
    double *d_w, *d_R, *d_cslot, *d_points, *d_order_xy, *d_rep_obs, *d_rep_base, *d_rep_info, *d_dep_meas, *d_dep_info, *d_arap_w;
    float *d_point_orig;
    int64_t *d_point_mpid, *d_arap_wk, *d_woff;
    unsigned long long *d_key;
    int32_t *d_ccnt, *d_cobs, *d_carap, *d_cenc, *d_sobs, *d_sarap, *d_senc, *d_enc, *d_encq, *d_first, *d_isfirst, *d_pnum, *d_slot_pt,
        *d_point_kf, *d_point_slot, *d_order_kf, *d_order_slot, *d_rep_point, *d_rep_cam, *d_dep_point, *d_dep_scale, *d_dep_cam,
        *d_arap_pts, *d_arap_pair, *d_arap_rot, *d_bsum, *d_ctl;
    DKf *d_kfs;
    DPair *d_pairs;
    int64_t geo_max = 1;
    for (const MeshIn &m : meshes) geo_max = std::max<int64_t>(geo_max, 6 * (int64_t)m.ntri);
    const int n_ctl = 8 + 2 * NM;      // [0] flags [1] geometry bad [4..7] counts [8 + m] nadj [8 + NM + m] non-identity map
    auto layout = [&](Bump &B) {
        for (int a = 0; a < K; a++) {
            if (!used[a]) continue;
            const deftri_keyframe &f = map.keyframes[a];
            dk[a].pid = B.take<int64_t>(f.n_slots);
            dk[a].pos = B.take<float>(3 * (size_t)f.n_slots);
            dk[a].obs = B.take<int32_t>(f.n_slots);
            dk[a].oct = B.take<int32_t>(f.n_obs);
            dk[a].uv = B.take<float>(2 * (size_t)f.n_obs);
            dk[a].depth = B.take<float>(f.n_obs);
            dk[a].meas = B.take<double>(f.n_obs);
            dk[a].status = B.take<uint8_t>(f.n_obs);
            dk[a].isig = B.take<float>(f.n_scales);
        }
        for (int m = 0; m < NM; m++) {
            const size_t n1 = (size_t)meshes[m].n1, c = 6 * (size_t)meshes[m].ntri;
            dm[m].pos = B.take<double>(3 * n1);
            dm[m].tris = B.take<int32_t>(3 * (size_t)meshes[m].ntri);
            dm[m].cnt = B.take<int32_t>(n1 + 1);
            dm[m].coff = B.take<int32_t>(n1 + 1);
            dm[m].cur = B.take<int32_t>(n1);
            dm[m].tmp = B.take<int32_t>(c);
            dm[m].ucnt = B.take<int32_t>(n1 + 1);
            dm[m].off = B.take<int32_t>(n1 + 1);
            dm[m].adj = B.take<int32_t>(c);
            dm[m].pos_idx = B.take<int32_t>(n1);
            dm[m].inv = B.take<int32_t>(n1);
            dm[m].bcnt = B.take<int32_t>(n1 + 1);
            dm[m].boff = B.take<int32_t>(n1 + 1);
            dm[m].bcur = B.take<int32_t>(n1);
            dm[m].items = B.take<int32_t>(n1);
        }
        for (int q = 0; q < NP; q++) dpos2[q] = B.take<double>(3 * (size_t)pairs[q].n2);
        B.take<double>(32);            // k_cot_finish mirrors a weight through csr_find: room in front of the weights
        d_w = B.take<double>(wsum);
        d_R = B.take<double>(9 * (size_t)n1sum);
        d_cslot = B.take<double>(2 * (size_t)geo_max);
        d_ccnt = B.take<int32_t>(geo_max);
        d_key = B.take<unsigned long long>(S);
        d_cobs = B.take<int32_t>(S + 1); d_carap = B.take<int32_t>(S + 1); d_cenc = B.take<int32_t>(S + 1);
        d_sobs = B.take<int32_t>(S + 1); d_sarap = B.take<int32_t>(S + 1); d_senc = B.take<int32_t>(S + 1);
        d_enc = B.take<int32_t>(S); d_encq = B.take<int32_t>(S);
        d_first = B.take<int32_t>(span);
        d_isfirst = B.take<int32_t>(cap_occ + 1); d_pnum = B.take<int32_t>(cap_occ + 1);
        d_slot_pt = B.take<int32_t>(2 * (size_t)S);
        d_point_mpid = B.take<int64_t>(cap_occ); d_points = B.take<double>(3 * (size_t)cap_occ);
        d_point_orig = B.take<float>(3 * (size_t)cap_occ); d_order_xy = B.take<double>(2 * (size_t)cap_occ);
        d_point_kf = B.take<int32_t>(cap_occ); d_point_slot = B.take<int32_t>(cap_occ);
        d_order_kf = B.take<int32_t>(cap_occ); d_order_slot = B.take<int32_t>(cap_occ);
        d_rep_point = B.take<int32_t>(2 * (size_t)cap_obs); d_rep_cam = B.take<int32_t>(2 * (size_t)cap_obs);
        d_rep_obs = B.take<double>(4 * (size_t)cap_obs); d_rep_base = B.take<double>(2 * (size_t)cap_obs);
        d_rep_info = B.take<double>(2 * (size_t)cap_obs);
        d_dep_point = B.take<int32_t>(2 * (size_t)cap_obs); d_dep_scale = B.take<int32_t>(2 * (size_t)cap_obs);
        d_dep_cam = B.take<int32_t>(2 * (size_t)cap_obs); d_dep_meas = B.take<double>(2 * (size_t)cap_obs);
        d_dep_info = B.take<double>(2 * (size_t)cap_obs);
        d_arap_pts = B.take<int32_t>(4 * (size_t)cap_arap); d_arap_pair = B.take<int32_t>(cap_arap);
        d_arap_rot = B.take<int32_t>(2 * (size_t)cap_arap); d_arap_w = B.take<double>(cap_arap);
        d_arap_wk = B.take<int64_t>(cap_arap);
        d_woff = B.take<int64_t>(NP);
        d_bsum = B.take<int32_t>((size_t)(scan_max / kScanTile) + 3);
        d_ctl = B.take<int32_t>(n_ctl);
        d_kfs = B.take<DKf>(K);
        d_pairs = B.take<DPair>(NP);
    };
    Bump sizing;
    layout(sizing);
    if (sizing.at > cap_) {
        if (buf_) { hipStreamSynchronize(st_); hipFree(buf_); buf_ = nullptr; cap_ = 0; }
        if (!check(hipMalloc(&buf_, sizing.at), "hipMalloc")) return -1;
        cap_ = sizing.at;
    }
    Bump B;
    B.base = static_cast<char *>(buf_);
    layout(B);
    for (hipEvent_t &e : ev_)
        if (!e && !check(hipEventCreate(&e), "hipEventCreate")) return -1;

    auto up = [&](void *dst, const void *src, size_t bytes) {
        if (!ok || bytes == 0) return;
        check(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st_), "upload");
        bytes_up += (int64_t)bytes;
    };
    auto zero = [&](void *dst, size_t bytes) {
        if (ok && bytes) check(hipMemsetAsync(dst, 0, bytes, st_), "memset");
    };
    auto scan = [&](const int32_t *in, int32_t *out, int64_t n) {
        const int nb = (int)std::max<int64_t>(1, (n + kScanTile - 1) / kScanTile);
        k_scan_tiles<<<nb, kB, 0, st_>>>(in, out, n, d_bsum);
        k_scan_sums<<<1, kB, 0, st_>>>(d_bsum, nb);
        k_scan_add<<<grid(n + 1), kB, 0, st_>>>(out, n, d_bsum, nb);
    };

    // the device views of the keyframes and the pairs
    std::vector<DKf> hkf((size_t)K, DKf{});
    for (int a = 0; a < K; a++) {
        if (!used[a]) continue;
        const deftri_keyframe &f = map.keyframes[a];
        const size_t ns = (size_t)f.n_slots, no = (size_t)f.n_obs;
        up(dk[a].pid, f.point_id, 8 * ns);
        up(dk[a].pos, f.point_pos, 12 * ns);
        up(dk[a].obs, f.obs_index, 4 * ns);
        up(dk[a].oct, f.kp_octave, 4 * no);
        up(dk[a].uv, f.kp_uv, 8 * no);
        if (dv[a].meas) up(dk[a].meas, dv[a].meas, 8 * no);
        else up(dk[a].depth, f.depth, 4 * no);
        if (dv[a].status) up(dk[a].status, dv[a].status, no);
        up(dk[a].isig, f.inv_sigma2, 4 * (size_t)f.n_scales);
        DKf &d = hkf[a];
        d.pid = dk[a].pid; d.pos = dk[a].pos; d.obs = dk[a].obs; d.oct = dk[a].oct; d.uv = dk[a].uv;
        d.depth = dv[a].meas ? nullptr : dk[a].depth;
        d.meas = dv[a].meas ? dk[a].meas : nullptr;
        d.status = dv[a].status ? dk[a].status : nullptr;
        d.isig = dk[a].isig;
        d.n_slots = f.n_slots; d.n_obs = f.n_obs; d.n_scales = f.n_scales;
    }
    std::vector<DPair> hp((size_t)NP);
    for (int q = 0; q < NP; q++) {
        const PairIn &p = pairs[q];
        DPair &d = hp[q];
        d.a = p.a; d.b = p.b; d.q = q; d.ns12 = p.ns12; d.n1 = meshes[p.mesh].n1; d.n2 = p.n2;
        d.c1 = p.c1; d.c2 = p.c2; d.s1 = p.s1; d.s2 = p.s2; d.rot_base = p.rot_base;
        d.sbase = sbase[q]; d.wpad = wpad[q];
        d.off = dm[p.mesh].off; d.adj = dm[p.mesh].adj; d.pos_idx = dm[p.mesh].pos_idx; d.inv = dm[p.mesh].inv;
        up(dpos2[q], p.pos2, 24 * (size_t)p.n2);
    }
    up(d_kfs, hkf.data(), sizeof(DKf) * (size_t)K);
    up(d_pairs, hp.data(), sizeof(DPair) * (size_t)NP);
    zero(d_ctl, sizeof(int32_t) * (size_t)n_ctl);
    if (!ok) return -1;
    int *flags = d_ctl, *geo_bad = d_ctl + 1;

    hipEventRecord(ev_[0], st_);
    // stage 0: the CSR adjacency of every mesh
    for (int m = 0; m < NM; m++) {
        const MeshIn &M = meshes[m];
        const int n1 = M.n1, ntri = M.ntri;
        const int64_t cap = 6 * (int64_t)ntri;
        up(dm[m].pos, M.pos1, 24 * (size_t)n1);
        up(dm[m].tris, M.tris, 12 * (size_t)ntri);
        zero(dm[m].cnt, 4 * (size_t)(n1 + 1));
        zero(dm[m].cur, 4 * (size_t)n1);
        k_adj_count<<<grid(3 * (int64_t)ntri), kB, 0, st_>>>(ntri, dm[m].tris, n1, dm[m].cnt, flags);
        scan(dm[m].cnt, dm[m].coff, n1);
        k_adj_fill<<<grid(ntri), kB, 0, st_>>>(ntri, dm[m].tris, n1, dm[m].coff, dm[m].cur, dm[m].tmp, cap);
        k_adj_sort<<<grid(n1, kSortBlock), kSortBlock, 0, st_>>>(n1, dm[m].coff, dm[m].tmp, dm[m].ucnt, flags);
        scan(dm[m].ucnt, dm[m].off, n1);
        k_adj_compact<<<grid(n1), kB, 0, st_>>>(n1, dm[m].coff, dm[m].off, dm[m].tmp, dm[m].adj, cap);
        k_mesh_count<<<1, 1, 0, st_>>>(dm[m].off, n1, d_ctl + 8 + m);
    }
    hipEventRecord(ev_[1], st_);
    // stage 1: the vector map of every mesh
    for (int m = 0; m < NM; m++) {
        const MeshIn &M = meshes[m];
        const int n1 = M.n1, nb = std::max(n1, 1);
        const double width = M.xmax - M.xmin;
        const double inv_h = width > 0 ? (double)nb / width : 0.0;
        zero(dm[m].bcnt, 4 * (size_t)(n1 + 1));
        zero(dm[m].bcur, 4 * (size_t)n1);
        k_bucket_count<<<grid(n1), kB, 0, st_>>>(n1, dm[m].pos, M.xmin, inv_h, nb, dm[m].bcnt);
        scan(dm[m].bcnt, dm[m].boff, nb);
        k_bucket_fill<<<grid(n1), kB, 0, st_>>>(n1, dm[m].pos, M.xmin, inv_h, nb, dm[m].boff, dm[m].bcur, dm[m].items);
        k_vector_map<<<grid(n1), kB, 0, st_>>>(n1, dm[m].pos, M.xmin, inv_h, nb, dm[m].boff, dm[m].items, dm[m].pos_idx,
                                               d_ctl + 8 + NM + m);
        k_fill_i32<<<grid(n1), kB, 0, st_>>>(dm[m].inv, n1, -1);
        k_inverse_map<<<grid(n1), kB, 0, st_>>>(n1, dm[m].pos_idx, dm[m].inv);
    }
    hipEventRecord(ev_[2], st_);
    // stage 2: the cot weights and the rotations of every pair, from the resident mesh
    for (int q = 0; q < NP; q++) {
        const PairIn &p = pairs[q];
        const MeshIn &M = meshes[p.mesh];
        zero(d_ccnt, 4 * (size_t)std::max<int64_t>(6 * (int64_t)M.ntri, 1));
        graph_geometry_launch(st_, M.n1, p.n2, M.ntri, dm[p.mesh].tris, dm[p.mesh].off, dm[p.mesh].adj, dm[p.mesh].pos_idx,
                              dm[p.mesh].inv, dm[p.mesh].pos, dpos2[q], d_cslot, d_ccnt, geo_bad, d_w + wpad[q],
                              d_R + 9 * (size_t)p.rot_base);
    }
    k_pair_offsets<<<1, 1, 0, st_>>>(d_pairs, NP, d_woff);
    hipEventRecord(ev_[3], st_);
    // stage 3: the slot scan of every pair, then the encounter order over the concatenated slots
    k_fill_u64<<<grid(S), kB, 0, st_>>>(d_key, S, ~0ULL);
    for (int q = 0; q < NP; q++)
        k_slot_scan<<<grid(hp[q].ns12), kB, 0, st_>>>(hkf[hp[q].b], hkf[hp[q].a], hp[q], d_key, d_cobs, d_carap, flags);
    for (int q = 0; q < NP; q++)
        k_enc<false><<<grid(hp[q].ns12), kB, 0, st_>>>(hkf[hp[q].b], hkf[hp[q].a], hp[q], d_key, d_cenc, nullptr, nullptr, nullptr, S);
    scan(d_cobs, d_sobs, S);
    scan(d_carap, d_sarap, S);
    scan(d_cenc, d_senc, S);
    for (int q = 0; q < NP; q++)
        k_enc<true><<<grid(hp[q].ns12), kB, 0, st_>>>(hkf[hp[q].b], hkf[hp[q].a], hp[q], d_key, nullptr, d_senc, d_enc, d_encq, S);
    hipEventRecord(ev_[4], st_);
    // stage 4: the points
    k_fill_i32<<<grid(span), kB, 0, st_>>>(d_first, span, INT32_MAX);
    if (ok && S > 0) check(hipMemsetAsync(d_slot_pt, 0xff, 8 * (size_t)S, st_), "memset");
    k_occ_first<<<grid(cap_occ), kB, 0, st_>>>(cap_occ, d_senc + S, d_enc, d_encq, d_pairs, NP, d_kfs, id_lo, span, d_first, flags);
    k_occ_flag<<<grid(cap_occ), kB, 0, st_>>>(cap_occ, d_senc + S, d_enc, d_encq, d_pairs, NP, d_kfs, id_lo, span, d_first, d_isfirst);
    scan(d_isfirst, d_pnum, cap_occ);
    k_occ_write<<<grid(cap_occ), kB, 0, st_>>>(cap_occ, d_senc + S, d_enc, d_encq, d_pairs, NP, d_kfs, id_lo, span, d_first, d_pnum,
                                               d_point_mpid, d_points, d_point_orig, d_order_xy, d_point_kf, d_point_slot,
                                               d_order_kf, d_order_slot, d_slot_pt);
    hipEventRecord(ev_[5], st_);
    // stage 5: the edges
    EdgeOut eo;
    eo.rep_point = d_rep_point; eo.rep_cam = d_rep_cam; eo.dep_point = d_dep_point; eo.dep_scale = d_dep_scale;
    eo.dep_cam = d_dep_cam; eo.arap_pts = d_arap_pts; eo.arap_pair = d_arap_pair; eo.arap_rot = d_arap_rot;
    eo.rep_obs = d_rep_obs; eo.rep_base = d_rep_base; eo.rep_info = d_rep_info; eo.dep_meas = d_dep_meas;
    eo.dep_info = d_dep_info; eo.arap_w = d_arap_w; eo.arap_wk = d_arap_wk;
    eo.cap_obs = cap_obs; eo.cap_arap = cap_arap;
    for (int q = 0; q < NP; q++)
        k_edges<<<grid(hp[q].ns12), kB, 0, st_>>>(hkf[hp[q].b], hkf[hp[q].a], hp[q], d_sobs, d_sarap, d_slot_pt, d_w, d_woff,
                                                  rep_weight, info_dep, eo);
    k_counts<<<1, 1, 0, st_>>>(d_senc + S, d_sobs + S, d_sarap + S, d_pnum + cap_occ, d_ctl);
    hipEventRecord(ev_[6], st_);
    if (!check(hipGetLastError(), "launch")) return -1;

    // the counts: one small download
    auto pin_need = [&](size_t bytes) {
        if (bytes <= pin_cap_) return true;
        if (pin_) { hipHostFree(pin_); pin_ = nullptr; pin_cap_ = 0; }
        if (!check(hipHostMalloc(&pin_, bytes), "hipHostMalloc")) return false;
        pin_cap_ = bytes;
        return true;
    };
    if (!pin_need(std::max<size_t>(4096, sizeof(int32_t) * (size_t)n_ctl))) return -1;
    if (!check(hipMemcpyAsync(pin_, d_ctl, sizeof(int32_t) * (size_t)n_ctl, hipMemcpyDeviceToHost, st_), "counts") ||
        !check(hipStreamSynchronize(st_), "synchronize"))
        return -1;
    syncs++;
    bytes_down += (int64_t)sizeof(int32_t) * n_ctl;
    std::vector<int32_t> ctl((int32_t *)pin_, (int32_t *)pin_ + n_ctl);
    for (int s = 0; s < 6; s++) {
        float ms = 0;
        hipEventElapsedTime(&ms, ev_[s], ev_[s + 1]);
        stage_ms[s] = ms;
    }
    if (ctl[0] & kFlagInput) { reason = 2; return 1; }
    if ((ctl[0] & (kFlagRow | kFlagIndex)) || ctl[1]) { reason = 3; return 1; }
    const int64_t nobs = ctl[5], narap = ctl[6], npts = ctl[7];
    if (nobs < 0 || nobs > cap_obs || narap < 0 || narap > cap_arap || npts < 0 || npts > cap_occ) { reason = 3; return 1; }
    for (int m = 0; m < NM; m++)
        if (ctl[8 + m] < 0 || ctl[8 + m] > 6 * (int64_t)meshes[m].ntri) { reason = 3; return 1; }

    // the arrays: one download through pinned staging
    struct Item { const void *src; void *dst; size_t bytes, at; };
    std::vector<Item> items;
    size_t total = 0;
    auto want = [&](const void *src, void *dst, size_t bytes) {
        if (!bytes) return;
        items.push_back({src, dst, bytes, total});
        total += align_up(bytes);
    };
    auto fetch = [&](auto &vec, const auto *src, size_t n) {
        vec.resize(n);
        want(src, vec.data(), sizeof(*src) * n);
    };
    for (int m = 0; m < NM; m++) {
        GraphResult::MeshData &md = *meshes[m].out;
        const size_t n1 = (size_t)meshes[m].n1;
        fetch(md.off, dm[m].off, n1 + 1);
        fetch(md.adj, dm[m].adj, (size_t)ctl[8 + m]);
        fetch(md.pos_idx, dm[m].pos_idx, n1);
        fetch(md.inv, dm[m].inv, n1);
        md.identity_map = md.skipped == 0 && ctl[8 + NM + m] == 0;
    }
    int64_t w_off = 0;
    g.wcat.clear();
    for (int q = 0; q < NP; q++) w_off += ctl[8 + pairs[q].mesh];
    g.wcat.resize((size_t)w_off);
    w_off = 0;
    for (int q = 0; q < NP; q++) {
        want(d_w + wpad[q], g.wcat.data() + w_off, 8 * (size_t)ctl[8 + pairs[q].mesh]);
        w_off += ctl[8 + pairs[q].mesh];
    }
    fetch(g.rot, d_R, 9 * (size_t)n1sum);
    fetch(g.point_mpid, d_point_mpid, (size_t)npts); fetch(g.points, d_points, 3 * (size_t)npts);
    fetch(g.point_orig, d_point_orig, 3 * (size_t)npts); fetch(g.order_xy, d_order_xy, 2 * (size_t)npts);
    fetch(g.point_kf, d_point_kf, (size_t)npts); fetch(g.point_slot, d_point_slot, (size_t)npts);
    fetch(g.order_kf, d_order_kf, (size_t)npts); fetch(g.order_slot, d_order_slot, (size_t)npts);
    fetch(g.rep_point, d_rep_point, 2 * (size_t)nobs); fetch(g.rep_cam, d_rep_cam, 2 * (size_t)nobs);
    fetch(g.rep_obs, d_rep_obs, 4 * (size_t)nobs); fetch(g.rep_base, d_rep_base, 2 * (size_t)nobs);
    fetch(g.rep_info, d_rep_info, 2 * (size_t)nobs);
    fetch(g.dep_point, d_dep_point, 2 * (size_t)nobs); fetch(g.dep_scale, d_dep_scale, 2 * (size_t)nobs);
    fetch(g.dep_cam, d_dep_cam, 2 * (size_t)nobs); fetch(g.dep_meas, d_dep_meas, 2 * (size_t)nobs);
    fetch(g.dep_info, d_dep_info, 2 * (size_t)nobs);
    fetch(g.arap_pts, d_arap_pts, 4 * (size_t)narap); fetch(g.arap_pair, d_arap_pair, (size_t)narap);
    fetch(g.arap_rot, d_arap_rot, 2 * (size_t)narap); fetch(g.arap_w, d_arap_w, (size_t)narap);
    fetch(g.arap_wk, d_arap_wk, (size_t)narap);
    if (!pin_need(std::max<size_t>(total, 4096))) return -1;
    for (const Item &it : items)
        if (!check(hipMemcpyAsync(static_cast<char *>(pin_) + it.at, it.src, it.bytes, hipMemcpyDeviceToHost, st_), "download"))
            return -1;
    if (!check(hipStreamSynchronize(st_), "synchronize")) return -1;
    syncs++;
    for (const Item &it : items) {
        std::memcpy(it.dst, static_cast<const char *>(pin_) + it.at, it.bytes);
        bytes_down += (int64_t)it.bytes;
    }
    return 0;
}

}  // namespace deftri
