// arap_deform.hip — the device path of deftri_arap_deform (arap_deform.h): every array stays on the device
// for the whole call (one upload, one download), one thread per vertex in every pass.
//   k_ad_local        the local step: R_i from the SVD of S_i (procrustes.h's Jacobi SVD, the matrix kept)
//   k_ad_rhs          the reduced right-hand side folded with the constraint term, and the warm start's
//                     residual r = b - A p, z = r / diag, d = z with the block partials of b.b, r.r, r.z
//   k_ad_begin        one block: the thresholds cg_tol^2 b.b and the flags of the initial residual
//   per CG iteration  k_ad_spmv (q = A d, partials of d.q), k_ad_update (alpha; p, r, z; partials of r.r and
//                     r.z), k_ad_dir (beta; d; block 0 writes the flags): three launches, the three
//                     coordinate columns in each, every column with its own alpha, beta and flag
//   k_ad_energy(_fin) the energy of the iterate
// A dot product is 256-thread block partials (a fixed tree in LDS) summed again by a fixed tree: k_ad_update
// and k_ad_dir sum the partials in every block, so no launch stands between a product and its use and no
// floating-point atomic is needed; two calls give the same bits.  A converged column is frozen by the flag
// the blocks derive from r.r alone, so the iterations the host launches past convergence (it reads the flags
// every kBatch iterations) change nothing, and the result does not depend on the batch size.
#include "arap_deform.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace deftri {
namespace arap {

namespace {

constexpr int kBlock = 256;
constexpr int kBatch = 32;          // CG iterations between two reads of the flags

struct CgState {
    double thr[3];                  // cg_tol^2 b.b per column
    int32_t conv[3];                // r.r <= thr
    int32_t done;                   // every column converged
    int32_t iters[3];               // CG iterations of this global step, per column
    int32_t err;                    // 1 det R <= 0, 2 a non-finite energy
};

// v[k] <- the sum over the block of v[k], in a fixed order, on every thread.  sh: K * kBlock doubles
template <int K>
__device__ inline void block_sum(double (&v)[K], double *sh) {
    const int t = threadIdx.x;
    for (int k = 0; k < K; k++) sh[k * kBlock + t] = v[k];
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int k = 0; k < K; k++) sh[k * kBlock + t] += sh[k * kBlock + t + s];
        __syncthreads();
    }
    for (int k = 0; k < K; k++) v[k] = sh[k * kBlock];
    __syncthreads();
}

// thread t's share of nblk partials of 3 values each: blocks t, t + kBlock, ... in order
__device__ inline void partial_share(const double *part, int nblk, double &a, double &b, double &c) {
    a = b = c = 0.0;
    for (int k = threadIdx.x; k < nblk; k += kBlock) { a += part[3 * k]; b += part[3 * k + 1]; c += part[3 * k + 2]; }
}

__global__ __launch_bounds__(kBlock) void k_ad_init(int n, const double *v, double *p, double *R) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < 3; c++) p[3 * (size_t)i + c] = v[3 * (size_t)i + c];
    for (int k = 0; k < 9; k++) R[9 * (size_t)i + k] = (k % 4 == 0) ? 1.0 : 0.0;
}

__global__ __launch_bounds__(kBlock) void k_ad_area(int ntri, const int32_t *tris, const double *v, double *part) {
    __shared__ double sh[kBlock];
    const int t = blockIdx.x * kBlock + threadIdx.x;
    double a[1] = {0.0};
    if (t < ntri) a[0] = tri_area(v + 3 * (size_t)tris[3 * t], v + 3 * (size_t)tris[3 * t + 1], v + 3 * (size_t)tris[3 * t + 2]);
    block_sum<1>(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a[0];
}

__global__ __launch_bounds__(kBlock) void k_ad_area_fin(int nblk, const double *part, double *area) {
    __shared__ double sh[kBlock];
    double a[1] = {0.0};
    for (int k = threadIdx.x; k < nblk; k += kBlock) a[0] += part[k];
    block_sum<1>(a, sh);
    if (threadIdx.x == 0) *area = a[0];
}

__global__ __launch_bounds__(kBlock) void k_ad_local(int n, const int32_t *off, const int32_t *adj, const double *w, const double *v,
                                                     const double *p, int smooth, double alpha, const double *area,
                                                     const double *Rold, double *R, CgState *st) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double smooth_c = smooth ? 4.0 * alpha * *area : 0.0;
    double Ri[9];
    const double det = local_rotation(i, off, adj, w, v, p, smooth_c, Rold, Ri);
    for (int k = 0; k < 9; k++) R[9 * (size_t)i + k] = Ri[k];
    if (!(det > 0.0)) atomicOr(&st->err, 1);
}

__global__ __launch_bounds__(kBlock) void k_ad_rhs(int n, const int32_t *off, const int32_t *adj, const double *w, const double *diag,
                                                   const int32_t *con, const double *cval, const double *v, double *p,
                                                   const double *R, double *r, double *z, double *d, double *part_bb,
                                                   double *part_rr, double *part_rz) {
    __shared__ double sh[9 * kBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (i < n) {
        if (con[i]) {
            // the own entry only: the other threads read a constrained vertex's position from cval
            for (int c = 0; c < 3; c++) {
                p[3 * (size_t)i + c] = cval[3 * (size_t)i + c];
                r[3 * (size_t)i + c] = z[3 * (size_t)i + c] = d[3 * (size_t)i + c] = 0.0;
            }
        } else {
            double b[3], Ap[3];
            rhs_row(i, off, adj, w, diag, con, cval, v, p, R, b, Ap);
            const double di = diag[i];
            for (int c = 0; c < 3; c++) {
                const double ri = b[c] - Ap[c], zi = ri / di;
                r[3 * (size_t)i + c] = ri; z[3 * (size_t)i + c] = zi; d[3 * (size_t)i + c] = zi;
                s[c] = b[c] * b[c]; s[3 + c] = ri * ri; s[6 + c] = ri * zi;
            }
        }
    }
    block_sum<9>(s, sh);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; c++) {
            part_bb[3 * blockIdx.x + c] = s[c];
            part_rr[3 * blockIdx.x + c] = s[3 + c];
            part_rz[3 * blockIdx.x + c] = s[6 + c];
        }
}

__global__ __launch_bounds__(kBlock) void k_ad_begin(int nblk, double tol2, const double *part_bb, const double *part_rr, CgState *st) {
    __shared__ double sh[6 * kBlock];
    double s[6];
    partial_share(part_bb, nblk, s[0], s[1], s[2]);
    partial_share(part_rr, nblk, s[3], s[4], s[5]);
    block_sum<6>(s, sh);
    if (threadIdx.x == 0) {
        int all = 1;
        for (int c = 0; c < 3; c++) {
            st->thr[c] = tol2 * s[c];
            st->conv[c] = s[3 + c] <= tol2 * s[c] ? 1 : 0;
            st->iters[c] = 0;
            all &= st->conv[c];
        }
        st->done = all;
    }
}

__global__ __launch_bounds__(kBlock) void k_ad_spmv(int n, const int32_t *off, const int32_t *adj, const double *w, const double *diag,
                                                    const int32_t *con, const double *d, double *q, double *part_dq) {
    __shared__ double sh[3 * kBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double s[3] = {0, 0, 0};
    if (i < n && !con[i]) {
        double qi[3];
        spmv_row(i, off, adj, w, diag, d, qi);
        for (int c = 0; c < 3; c++) { q[3 * (size_t)i + c] = qi[c]; s[c] = d[3 * (size_t)i + c] * qi[c]; }
    }
    block_sum<3>(s, sh);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; c++) part_dq[3 * blockIdx.x + c] = s[c];
}

// alpha = r.z / d.q from the partials, then p += alpha d, r -= alpha q, z = r / diag and the new partials; a
// converged column keeps p, r and z, so its partials repeat
__global__ __launch_bounds__(kBlock) void k_ad_update(int n, int nblk, const int32_t *con, const double *diag, const double *d,
                                                      const double *q, double *p, double *r, double *z, const double *part_dq,
                                                      const double *part_rz_cur, double *part_rr_next, double *part_rz_next,
                                                      CgState *st) {
    __shared__ double sh[6 * kBlock];
    double s[6];
    partial_share(part_dq, nblk, s[0], s[1], s[2]);
    partial_share(part_rz_cur, nblk, s[3], s[4], s[5]);
    block_sum<6>(s, sh);
    int conv[3];
    double a[3];
    for (int c = 0; c < 3; c++) { conv[c] = st->conv[c]; a[c] = conv[c] ? 0.0 : s[3 + c] / s[c]; }
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double o[6] = {0, 0, 0, 0, 0, 0};
    if (i < n && !con[i]) {
        const double di = diag[i];
        for (int c = 0; c < 3; c++) {
            const size_t at = 3 * (size_t)i + c;
            double ri = r[at], zi = z[at];
            if (!conv[c]) {
                p[at] += a[c] * d[at];
                ri -= a[c] * q[at];
                zi = ri / di;
                r[at] = ri;
                z[at] = zi;
            }
            o[c] = ri * ri;
            o[3 + c] = ri * zi;
        }
    }
    block_sum<6>(o, sh);
    if (threadIdx.x == 0) {
        for (int c = 0; c < 3; c++) { part_rr_next[3 * blockIdx.x + c] = o[c]; part_rz_next[3 * blockIdx.x + c] = o[3 + c]; }
        if (blockIdx.x == 0)
            for (int c = 0; c < 3; c++)
                if (!conv[c]) st->iters[c]++;
    }
}

// the flags of the new residual, beta = r.z new / r.z old, d = z + beta d for the columns still running
__global__ __launch_bounds__(kBlock) void k_ad_dir(int n, int nblk, const int32_t *con, const double *z, double *d,
                                                   const double *part_rr_next, const double *part_rz_next,
                                                   const double *part_rz_cur, CgState *st) {
    __shared__ double sh[9 * kBlock];
    double s[9];
    partial_share(part_rr_next, nblk, s[0], s[1], s[2]);
    partial_share(part_rz_next, nblk, s[3], s[4], s[5]);
    partial_share(part_rz_cur, nblk, s[6], s[7], s[8]);
    block_sum<9>(s, sh);
    int conv[3];
    for (int c = 0; c < 3; c++) conv[c] = s[c] <= st->thr[c] ? 1 : 0;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n && !con[i])
        for (int c = 0; c < 3; c++)
            if (!conv[c]) {
                const size_t at = 3 * (size_t)i + c;
                d[at] = z[at] + (s[3 + c] / s[6 + c]) * d[at];
            }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int c = 0; c < 3; c++) st->conv[c] = conv[c];
        st->done = conv[0] & conv[1] & conv[2];
    }
}

__global__ __launch_bounds__(kBlock) void k_ad_energy(int n, const int32_t *off, const int32_t *adj, const double *w, const double *v,
                                                      const double *p, const double *R, int smoothed, double *part_e) {
    __shared__ double sh[2 * kBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double s[2] = {0, 0};
    if (i < n) energy_vertex(i, off, adj, w, v, p, R, smoothed != 0, s[0], s[1]);
    block_sum<2>(s, sh);
    if (threadIdx.x == 0) { part_e[2 * blockIdx.x] = s[0]; part_e[2 * blockIdx.x + 1] = s[1]; }
}

__global__ __launch_bounds__(kBlock) void k_ad_energy_fin(int nblk, const double *part_e, int smoothed, double alpha, const double *area,
                                                          double *energy, CgState *st) {
    __shared__ double sh[2 * kBlock];
    double s[2] = {0, 0};
    for (int k = threadIdx.x; k < nblk; k += kBlock) { s[0] += part_e[2 * k]; s[1] += part_e[2 * k + 1]; }
    block_sum<2>(s, sh);
    if (threadIdx.x == 0) {
        const double E = smoothed ? s[0] + alpha * *area * s[1] : s[0];
        *energy = E;
        if (!isfinite(E)) atomicOr(&st->err, 2);
    }
}

// a bump allocator over one device buffer and its host mirror of the uploaded prefix
struct Layout {
    size_t size = 0;
    size_t take(size_t bytes) {
        const size_t at = size;
        size = (size + bytes + 255) & ~(size_t)255;
        return at;
    }
};

}  // namespace

int run_device(int device, hipStream_t st, const System &S, double *out, double *energies, deftri_arap_deform_report *rep,
               std::string &err) {
    const int n = S.n, ntri = S.ntri, nblk = (n + kBlock - 1) / kBlock, nblk_t = std::max(1, (ntri + kBlock - 1) / kBlock);
    const size_t nnz = S.adj.size();
    const int smoothed = S.energy == 1;
    int batch = kBatch;
    if (const char *e = std::getenv("DEFTRI_ARAP_CG_BATCH")) batch = std::max(1, std::atoi(e));   // tests: the result does not depend on it
    auto fail = [&](const char *what, hipError_t e) {
        err = std::string("arap_deform: ") + what + ": " + hipGetErrorString(e);
        return DEFTRI_E_HIP;
    };
    hipError_t he = hipSetDevice(device);
    if (he != hipSuccess) return fail("hipSetDevice", he);
    const size_t D = sizeof(double), I = sizeof(int32_t);
    Layout L;
    // the uploaded prefix
    const size_t o_v = L.take(3 * (size_t)n * D), o_cval = L.take(3 * (size_t)n * D), o_w = L.take(std::max<size_t>(nnz, 1) * D),
                 o_diag = L.take((size_t)n * D), o_off = L.take(((size_t)n + 1) * I), o_adj = L.take(std::max<size_t>(nnz, 1) * I),
                 o_con = L.take((size_t)n * I), o_tris = L.take(std::max<size_t>(3 * (size_t)ntri, 1) * I), o_st = L.take(sizeof(CgState));
    const size_t up_bytes = L.size;
    // the downloaded block: p, energies, area
    const size_t o_p = L.take((3 * (size_t)n + (size_t)S.max_iter + 1) * D);
    const size_t dn_bytes = (3 * (size_t)n + (size_t)S.max_iter + 1) * D;
    const size_t o_R = L.take(9 * (size_t)n * D), o_R2 = smoothed ? L.take(9 * (size_t)n * D) : o_R;
    const size_t o_r = L.take(3 * (size_t)n * D), o_z = L.take(3 * (size_t)n * D), o_d = L.take(3 * (size_t)n * D),
                 o_q = L.take(3 * (size_t)n * D);
    const size_t o_pdq = L.take(3 * (size_t)nblk * D), o_pbb = L.take(3 * (size_t)nblk * D), o_prr0 = L.take(3 * (size_t)nblk * D),
                 o_prr1 = L.take(3 * (size_t)nblk * D), o_prz0 = L.take(3 * (size_t)nblk * D), o_prz1 = L.take(3 * (size_t)nblk * D),
                 o_pe = L.take(2 * (size_t)nblk * D), o_pa = L.take((size_t)nblk_t * D);
    char *dev = nullptr, *pin = nullptr;
    hipEvent_t ev[2][3] = {};
    auto release = [&]() {
        for (auto &row : ev)
            for (hipEvent_t &e : row)
                if (e) hipEventDestroy(e);
        if (dev) hipFree(dev);
        if (pin) hipHostFree(pin);
    };
    const size_t pin_bytes = ((std::max(up_bytes, dn_bytes) + 255) & ~(size_t)255) + 256;
    if ((he = hipMalloc((void **)&dev, L.size)) != hipSuccess) { release(); return fail("hipMalloc", he); }
    if ((he = hipHostMalloc((void **)&pin, pin_bytes)) != hipSuccess) { release(); return fail("hipHostMalloc", he); }
    for (auto &row : ev)
        for (hipEvent_t &e : row)
            if ((he = hipEventCreate(&e)) != hipSuccess) { release(); return fail("hipEventCreate", he); }
    std::memset(pin, 0, up_bytes);
    std::memcpy(pin + o_v, S.v.data(), 3 * (size_t)n * D);
    std::memcpy(pin + o_cval, S.cval.data(), 3 * (size_t)n * D);
    if (nnz) std::memcpy(pin + o_w, S.w.data(), nnz * D);
    std::memcpy(pin + o_diag, S.diag.data(), (size_t)n * D);
    std::memcpy(pin + o_off, S.off.data(), ((size_t)n + 1) * I);
    if (nnz) std::memcpy(pin + o_adj, S.adj.data(), nnz * I);
    std::memcpy(pin + o_con, S.con.data(), (size_t)n * I);
    if (ntri) std::memcpy(pin + o_tris, S.tris.data(), 3 * (size_t)ntri * I);
    if ((he = hipMemcpyAsync(dev, pin, up_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) { release(); return fail("upload", he); }
    // the flags travel through their own small pinned block, so the upload's mirror is free at once
    CgState *hst = reinterpret_cast<CgState *>(pin + pin_bytes - 256);
    std::memset(hst, 0, sizeof(CgState));
    const double *v = (const double *)(dev + o_v), *cval = (const double *)(dev + o_cval), *w = (const double *)(dev + o_w),
                 *diag = (const double *)(dev + o_diag);
    const int32_t *off = (const int32_t *)(dev + o_off), *adj = (const int32_t *)(dev + o_adj), *con = (const int32_t *)(dev + o_con),
                  *tris = (const int32_t *)(dev + o_tris);
    CgState *dst = (CgState *)(dev + o_st);
    double *p = (double *)(dev + o_p), *den = p + 3 * (size_t)n, *darea = den + S.max_iter;
    double *Ra = (double *)(dev + o_R), *Rb = (double *)(dev + o_R2);
    double *r = (double *)(dev + o_r), *z = (double *)(dev + o_z), *d = (double *)(dev + o_d), *q = (double *)(dev + o_q);
    double *pdq = (double *)(dev + o_pdq), *pbb = (double *)(dev + o_pbb), *pe = (double *)(dev + o_pe), *pa = (double *)(dev + o_pa);
    double *prr[2] = {(double *)(dev + o_prr0), (double *)(dev + o_prr1)}, *prz[2] = {(double *)(dev + o_prz0), (double *)(dev + o_prz1)};

    k_ad_init<<<nblk, kBlock, 0, st>>>(n, v, p, Ra);
    if (smoothed) k_ad_init<<<nblk, kBlock, 0, st>>>(n, v, p, Rb);
    k_ad_area<<<nblk_t, kBlock, 0, st>>>(ntri, tris, v, pa);
    k_ad_area_fin<<<1, kBlock, 0, st>>>(nblk_t, pa, darea);
    auto read_state = [&]() -> hipError_t {
        hipError_t e = hipMemcpyAsync(hst, dst, sizeof(CgState), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return e;
        return hipStreamSynchronize(st);
    };
    int rc = 0;
    double *Rcur = Ra, *Rold = Rb;
    float ms = 0;
    int ended = -1;                 // the last iteration whose end event was recorded
    for (int it = 0; it < S.max_iter && rc == 0; it++) {
        hipEvent_t *e3 = ev[it & 1];
        if (smoothed) std::swap(Rcur, Rold);
        hipEventRecord(e3[0], st);
        k_ad_local<<<nblk, kBlock, 0, st>>>(n, off, adj, w, v, p, smoothed && it > 0, S.alpha, darea, Rold, Rcur, dst);
        hipEventRecord(e3[1], st);
        k_ad_rhs<<<nblk, kBlock, 0, st>>>(n, off, adj, w, diag, con, cval, v, p, Rcur, r, z, d, pbb, prr[0], prz[0]);
        k_ad_begin<<<1, kBlock, 0, st>>>(nblk, S.tol * S.tol, pbb, prr[0], dst);
        if ((he = read_state()) != hipSuccess) { rc = fail("global step", he); break; }
        if (hipEventElapsedTime(&ms, e3[0], e3[1]) == hipSuccess) rep->ms_local += ms;
        if (ended == it - 1 && it > 0 && hipEventElapsedTime(&ms, ev[ended & 1][1], ev[ended & 1][2]) == hipSuccess) rep->ms_global += ms;
        if (hst->err) break;
        int launched = 0;
        while (!hst->done && launched < S.cg_max) {
            const int nb = std::min(batch, S.cg_max - launched);
            for (int k = 0; k < nb; k++) {
                const int cur = (launched + k) & 1, nxt = cur ^ 1;
                k_ad_spmv<<<nblk, kBlock, 0, st>>>(n, off, adj, w, diag, con, d, q, pdq);
                k_ad_update<<<nblk, kBlock, 0, st>>>(n, nblk, con, diag, d, q, p, r, z, pdq, prz[cur], prr[nxt], prz[nxt], dst);
                k_ad_dir<<<nblk, kBlock, 0, st>>>(n, nblk, con, z, d, prr[nxt], prz[nxt], prz[cur], dst);
            }
            launched += nb;
            if ((he = read_state()) != hipSuccess) { rc = fail("CG batch", he); break; }
        }
        if (rc) break;
        const int mx = std::max(hst->iters[0], std::max(hst->iters[1], hst->iters[2]));
        rep->cg_iterations += (int64_t)hst->iters[0] + hst->iters[1] + hst->iters[2];
        rep->cg_max_in_step = std::max(rep->cg_max_in_step, mx);
        rep->iterations = it + 1;
        if (!hst->done) {
            rep->cg_unconverged_steps++;
            err = "arap_deform: the global step of iteration " + std::to_string(it + 1) + " did not reach cg_tol within " +
                  std::to_string(S.cg_max) + " CG iterations";
            rc = DEFTRI_E_NUMERIC;
            break;
        }
        k_ad_energy<<<nblk, kBlock, 0, st>>>(n, off, adj, w, v, p, Rcur, smoothed, pe);
        k_ad_energy_fin<<<1, kBlock, 0, st>>>(nblk, pe, smoothed, S.alpha, darea, den + it, dst);
        hipEventRecord(e3[2], st);
        ended = it;
    }
    if (rc == 0) {
        // one download: p, the energies, the area; the flags once more for the last energy
        he = hipMemcpyAsync(pin, p, dn_bytes, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = read_state();
        if (he == hipSuccess) he = hipGetLastError();
        if (he != hipSuccess) rc = fail("download", he);
    }
    if (rc == 0) {
        if (ended >= 0 && ended == rep->iterations - 1 && hipEventElapsedTime(&ms, ev[ended & 1][1], ev[ended & 1][2]) == hipSuccess)
            rep->ms_global += ms;
        const double *hp = (const double *)pin, *hen = hp + 3 * (size_t)n;
        rep->area = hen[S.max_iter];
        if (hst->err & 1) { err = "arap_deform: det R <= 0 in a local step"; rc = DEFTRI_E_NUMERIC; }
        else if (hst->err & 2) { err = "arap_deform: non-finite iterate"; rc = DEFTRI_E_NUMERIC; }
        for (size_t k = 0; k < 3 * (size_t)n && rc == 0; k++)
            if (!std::isfinite(hp[k])) { err = "arap_deform: non-finite iterate"; rc = DEFTRI_E_NUMERIC; }
        if (rc == 0) {
            if (S.max_iter > 0) { rep->energy_first = hen[0]; rep->energy_last = hen[S.max_iter - 1]; }
            std::memcpy(out, hp, 3 * (size_t)n * D);
            if (energies) std::memcpy(energies, hen, (size_t)S.max_iter * D);
        }
    } else {
        hipStreamSynchronize(st);
    }
    release();
    return rc;
}

}  // namespace arap
}  // namespace deftri
