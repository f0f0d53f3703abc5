// essential.hip — the second pose from the matches alone: findEssentialWithRANSAC with a model per
// iteration and reconstructCameras (reference Modules/Mapping/MonocularMapInitializer.cc:119-279).
//
// The reference draws 8 matches per iteration (one from each of 8 k-means clusters, :128-155), would fit
// E to them (computeE, :180-203; the call is commented out at :158), scores E against every match
// (computeScoreAndInliers, :206-223) and keeps the first E of the highest score (:167-171).  The draws
// are the caller's (`samples`); everything after them is here, all hypotheses at once:
//   k_rays              one thread per match: both unit rays (:79-80), once, as six float arrays
//   k_essential_models  one thread per hypothesis: the null vector of the 8 x 9 system and the rank-2
//                       projection U diag(1,1,0) V^T, in fp64, rounded to float at the end
//   k_score             n_hyp x n evaluations: a thread holds one match's rays, a workgroup walks a tile of
//                       64 hypotheses whose E sit in LDS; counts by ballot, one integer atomicAdd per wave
//                       and hypothesis
//   k_best              one workgroup: the lowest index among the highest scores, then the mask and the
//                       errors of that E
// reconstructCameras (:246-262): decomposeE (:264-279) of the given E on the host in fp64, then
//   k_camera_vote       one thread per match: sign((Rgood r1 - r2) . (r2 - t)), summed as integers
//
// Closed forms instead of the two JacobiSVDs: an 8 x 9 matrix of rank 8 has an exact
// one-dimensional null space, found by elimination with complete pivoting; U diag(1,1,0) V^T of the 3 x 3 e
// is e (v1 v1^T / s1 + v2 v2^T / s2) with (s_i^2, v_i) the two largest eigenpairs of e^T e, from cyclic
// Jacobi rotations.  Only + - * / sqrt, without contraction, so the host loops and the kernels round
// alike; the rays differ where the two libm's sinf / cosf do.
//
// One upload (pixels and samples) and one download (every output) per call.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "dev_arena.h"
#include "device_math.h"
#include "epipolar.h"
#include "essential.h"

namespace deftri {

namespace dev {

constexpr int TILE_H = 64;         // hypotheses per k_score workgroup
constexpr int MODEL_THREADS = 64;  // hypotheses per k_essential_models workgroup
constexpr int WORK = 81;           // doubles of work space per hypothesis: A (8 x 9) and the solution (9)

// what k_best leaves at the head of the download
struct RansacHead {
    float E_best[9];
    int best, best_score, n_degenerate;
};

// a permutation of 0..8 in the nibbles of a 64-bit word
__host__ __device__ __forceinline__ int nib(unsigned long long p, int j) { return (int)((p >> (4 * j)) & 15ull); }
__host__ __device__ __forceinline__ unsigned long long nib_swap(unsigned long long p, int a, int b) {
    const unsigned long long x = ((p >> (4 * a)) ^ (p >> (4 * b))) & 15ull;
    return p ^ (x << (4 * a)) ^ (x << (4 * b));
}

__host__ __device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.4028234663852886e38f; }

// one Jacobi rotation of the symmetric 3 x 3 (app, aqq, apq, and the third index r) that zeroes apq; the
// eigenvector columns p and q of V (row-major 3 x 3) rotate with it
__host__ __device__ __forceinline__ void jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double *V,
                                                       int p, int q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double vp = V[3 * k + p], vq = V[3 * k + q];
        V[3 * k + p] = c * vp - s * vq;
        V[3 * k + q] = s * vp + c * vq;
    }
}

// eigenvalues (descending) and eigenvectors (the columns of V, row-major) of e^T e for a row-major 3 x 3 e
__host__ __device__ __forceinline__ void gram_eigen(const double *e, double *lam, double *V) {
    double m00 = e[0] * e[0] + e[3] * e[3] + e[6] * e[6], m11 = e[1] * e[1] + e[4] * e[4] + e[7] * e[7];
    double m22 = e[2] * e[2] + e[5] * e[5] + e[8] * e[8], m01 = e[0] * e[1] + e[3] * e[4] + e[6] * e[7];
    double m02 = e[0] * e[2] + e[3] * e[5] + e[6] * e[8], m12 = e[1] * e[2] + e[4] * e[5] + e[7] * e[8];
#pragma unroll
    for (int k = 0; k < 9; k++) V[k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 8; sweep++) {
        jacobi_rotate(m00, m11, m01, m02, m12, V, 0, 1);
        jacobi_rotate(m00, m22, m02, m01, m12, V, 0, 2);
        jacobi_rotate(m11, m22, m12, m01, m02, V, 1, 2);
    }
    lam[0] = m00; lam[1] = m11; lam[2] = m22;
#define DEFTRI_SORT2(a, b)                                                                   \
    if (lam[b] > lam[a]) {                                                                   \
        const double l_ = lam[a]; lam[a] = lam[b]; lam[b] = l_;                              \
        for (int k = 0; k < 3; k++) { const double v_ = V[3 * k + a]; V[3 * k + a] = V[3 * k + b]; V[3 * k + b] = v_; } \
    }
    DEFTRI_SORT2(0, 1)
    DEFTRI_SORT2(0, 2)
    DEFTRI_SORT2(1, 2)
#undef DEFTRI_SORT2
}

// computeE (:180-203) for the 8 matches idx[0..8) of the ray arrays (rays[c * n + i]: c = 0..2 the first
// view's ray, 3..5 the second's).  W: WORK doubles at stride `s`.  E [9] row-major; false (and E zero): a
// degenerate sample (deftri.h).  The indices are inside [0, n).
__host__ __device__ inline bool essential_model(const float *rays, int n, const int *idx, double *W, int s, float *E) {
#pragma unroll
    for (int k = 0; k < 9; k++) E[k] = 0.0f;
    for (int i = 0; i < 8; i++)
        for (int j = i + 1; j < 8; j++)
            if (idx[i] == idx[j]) return false;
    // A (:183-187): row i = [r1 * r2.x, r1 * r2.y, r1 * r2.z]; a product of two floats is exact in fp64
    for (int i = 0; i < 8; i++) {
        double r[6];
        bool fin = true;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const float v = rays[(size_t)c * n + idx[i]];
            fin = fin && finite_f(v);
            r[c] = (double)v;
        }
        if (!fin) return false;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) W[(9 * i + 3 * a + b) * s] = r[b] * r[3 + a];
    }
    // elimination with complete pivoting: the largest remaining entry, the lowest (row, column) on ties
    unsigned long long cp = 0x876543210ull;                  // column j of the work matrix is column nib(cp, j) of A
    for (int k = 0; k < 8; k++) {
        double big = 0.0;
        int pi = k, pj = k;
        for (int i = k; i < 8; i++)
            for (int j = k; j < 9; j++) {
                const double a = fabs(W[(9 * i + j) * s]);
                if (a > big) { big = a; pi = i; pj = j; }
            }
        if (!(big > 0.0)) return false;                      // a zero pivot: rank below 8
        if (pi != k)
            for (int j = k; j < 9; j++) {
                const double t = W[(9 * k + j) * s];
                W[(9 * k + j) * s] = W[(9 * pi + j) * s];
                W[(9 * pi + j) * s] = t;
            }
        if (pj != k) {
            for (int i = 0; i < 8; i++) {
                const double t = W[(9 * i + k) * s];
                W[(9 * i + k) * s] = W[(9 * i + pj) * s];
                W[(9 * i + pj) * s] = t;
            }
            cp = nib_swap(cp, k, pj);
        }
        const double piv = W[(9 * k + k) * s];
        for (int i = k + 1; i < 8; i++) {
            const double f = W[(9 * i + k) * s] / piv;
            for (int j = k + 1; j < 9; j++) W[(9 * i + j) * s] = W[(9 * i + j) * s] - f * W[(9 * k + j) * s];
        }
    }
    // back substitution with the free unknown 1: x in row 8 of the work space
    W[(72 + 8) * s] = 1.0;
    for (int k = 7; k >= 0; k--) {
        double acc = 0.0;
        for (int j = k + 1; j < 9; j++) acc = acc + W[(9 * k + j) * s] * W[(72 + j) * s];
        W[(72 + k) * s] = -acc / W[(9 * k + k) * s];
    }
    unsigned long long inv = 0;
    for (int j = 0; j < 9; j++) inv |= (unsigned long long)j << (4 * nib(cp, j));
    double e[9];
#pragma unroll
    for (int c = 0; c < 9; c++) e[c] = W[(72 + nib(inv, c)) * s];
    // the sign (deftri.h): the component of largest magnitude is positive, the lowest index on ties; scaled to 1
    double big = 0.0, lead = 1.0;
#pragma unroll
    for (int c = 0; c < 9; c++)
        if (fabs(e[c]) > big) { big = fabs(e[c]); lead = e[c]; }
    if (!(big > 0.0) || !(big <= 1.7976931348623157e308)) return false;
#pragma unroll
    for (int c = 0; c < 9; c++) e[c] = e[c] / lead;
    // Ef = U diag(1, 1, 0) V^T (:197-200) = e (v1 v1^T / s1 + v2 v2^T / s2)
    double lam[3], V[9];
    gram_eigen(e, lam, V);
    if (!(lam[1] > 0.0)) return false;                       // sigma_2 == 0
    const double s1 = sqrt(lam[0]), s2 = sqrt(lam[1]);
    double P[9];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) P[3 * a + b] = V[3 * a] * V[3 * b] / s1 + V[3 * a + 1] * V[3 * b + 1] / s2;
    float out[9];
    bool fin = true;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            const double ef = e[3 * a] * P[b] + e[3 * a + 1] * P[3 + b] + e[3 * a + 2] * P[6 + b];
            out[3 * a + b] = (float)(-ef);                   // :202
            fin = fin && finite_f(out[3 * a + b]);
        }
    if (!fin) return false;
#pragma unroll
    for (int k = 0; k < 9; k++) E[k] = out[k];
    return true;
}

// sign(((Rgood r1 - r2) . (r2 - t))) (:256-257): R row-major 3 x 3, in float; 0 for a zero or a NaN
__host__ __device__ __forceinline__ int camera_vote(const float *R, const float *t, V3 r1, V3 r2) {
    const V3 a = sub(v3(dot(v3(R[0], R[1], R[2]), r1), dot(v3(R[3], R[4], R[5]), r1), dot(v3(R[6], R[7], R[8]), r1)), r2);
    const V3 b = sub(r2, v3(t[0], t[1], t[2]));
    const float s = dot(a, b);
    return (s > 0.0f) - (s < 0.0f);
}

__global__ void __launch_bounds__(256)
k_rays(int n, const float *__restrict__ uv1, const float *__restrict__ uv2, Kb8 k1, Kb8 k2, float *__restrict__ rays) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    V3 r1, r2;
    epipolar_rays(k1, k2, uv1[2 * i], uv1[2 * i + 1], uv2[2 * i], uv2[2 * i + 1], r1, r2);
    const size_t N = (size_t)n;
    rays[i] = r1.x; rays[N + i] = r1.y; rays[2 * N + i] = r1.z;
    rays[3 * N + i] = r2.x; rays[4 * N + i] = r2.y; rays[5 * N + i] = r2.z;
}

// one thread per hypothesis; its work space is a column of LDS (stride MODEL_THREADS: no bank conflicts
// between the lanes, and the pivot search indexes it dynamically)
__global__ void __launch_bounds__(MODEL_THREADS)
k_essential_models(int n, int n_hyp, const float *__restrict__ rays, const int *__restrict__ samples, float *__restrict__ E_all,
                   uint8_t *__restrict__ degenerate, int *__restrict__ n_degenerate) {
    __shared__ double work[WORK * MODEL_THREADS];
    const int h = (int)(blockIdx.x * MODEL_THREADS + threadIdx.x);
    bool bad = false;
    if (h < n_hyp) {
        int idx[8];
#pragma unroll
        for (int k = 0; k < 8; k++) idx[k] = samples[8 * (size_t)h + k];
        float E[9];
        bad = !essential_model(rays, n, idx, work + threadIdx.x, MODEL_THREADS, E);
#pragma unroll
        for (int k = 0; k < 9; k++) E_all[9 * (size_t)h + k] = E[k];
        degenerate[h] = bad ? 1 : 0;
    }
    const unsigned long long m = __ballot(bad);
    if (threadIdx.x == 0 && m) atomicAdd(n_degenerate, __popcll(m));
}

// grid (match blocks, hypothesis tiles).  A degenerate hypothesis is not scored: its score stays 0.
__global__ void __launch_bounds__(256)
k_score(int n, int n_hyp, const float *__restrict__ rays, const float *__restrict__ E_all, const uint8_t *__restrict__ degenerate,
        float th, int *__restrict__ scores) {
    __shared__ float sE[9 * TILE_H];
    __shared__ uint8_t sDeg[TILE_H];
    const int h0 = (int)blockIdx.y * TILE_H;
    const int nh = min(TILE_H, n_hyp - h0);
    for (int k = (int)threadIdx.x; k < 9 * nh; k += 256) sE[k] = E_all[9 * (size_t)h0 + k];
    for (int k = (int)threadIdx.x; k < nh; k += 256) sDeg[k] = degenerate[h0 + k];
    __syncthreads();
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const bool live = i < n;
    V3 r1 = v3(0.0f, 0.0f, 0.0f), r2n = r1;
    if (live) {
        const size_t N = (size_t)n;
        r1 = v3(rays[i], rays[N + i], rays[2 * N + i]);
        r2n = eigen_normalized(v3(rays[3 * N + i], rays[4 * N + i], rays[5 * N + i]));
    }
    for (int k = 0; k < nh; k++) {
        if (sDeg[k]) continue;                                // uniform over the workgroup
        const bool in = live && epipolar_score(sE + 9 * k, r1, r2n) < th;     // :211
        const unsigned long long m = __ballot(in);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&scores[h0 + k], __popcll(m));
    }
}

// one workgroup: bestScore starts at 0 and is replaced on score > bestScore (:120, :167), so the best is
// the lowest index among the highest scores and none when every score is 0; then computeScoreAndInliers
// of that E for the mask and the errors (NaN where there is no best)
__global__ void __launch_bounds__(256)
k_best(int n, int n_hyp, const float *__restrict__ rays, const float *__restrict__ E_all, const int *__restrict__ scores, float th,
       RansacHead *__restrict__ head, uint8_t *__restrict__ inlier, float *__restrict__ err) {
    __shared__ int sScore[256], sIdx[256];
    __shared__ float sE[9];
    int bs = 0, bi = -1;
    for (int h = (int)threadIdx.x; h < n_hyp; h += 256) {
        const int s = scores[h];
        if (s > bs) { bs = s; bi = h; }                       // ascending h: the first of the highest
    }
    sScore[threadIdx.x] = bs;
    sIdx[threadIdx.x] = bi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const int s2 = sScore[threadIdx.x + off], i2 = sIdx[threadIdx.x + off];
            const int s1 = sScore[threadIdx.x], i1 = sIdx[threadIdx.x];
            if (s2 > s1 || (s2 == s1 && s2 > 0 && i2 < i1)) { sScore[threadIdx.x] = s2; sIdx[threadIdx.x] = i2; }
        }
        __syncthreads();
    }
    const int best = sIdx[0];
    if (threadIdx.x < 9) {
        const float v = best >= 0 ? E_all[9 * (size_t)best + threadIdx.x] : 0.0f;
        sE[threadIdx.x] = v;
        head->E_best[threadIdx.x] = v;
    }
    if (threadIdx.x == 0) { head->best = best; head->best_score = sScore[0]; }
    __syncthreads();
    const size_t N = (size_t)n;
    for (int i = (int)threadIdx.x; i < n; i += 256) {
        if (best < 0) {
            inlier[i] = 0;
            err[i] = __builtin_nanf("");
            continue;
        }
        const V3 r1 = v3(rays[i], rays[N + i], rays[2 * N + i]);
        const V3 r2n = eigen_normalized(v3(rays[3 * N + i], rays[4 * N + i], rays[5 * N + i]));
        const float e = epipolar_score(sE, r1, r2n);
        inlier[i] = e < th ? 1 : 0;
        err[i] = e;
    }
}

// away (:256-257) over the used matches: a ballot of the positive and of the negative votes per wave, one
// integer atomicAdd per wave
__global__ void __launch_bounds__(256)
k_camera_vote(int n, const float *__restrict__ uv1, const float *__restrict__ uv2, const uint8_t *__restrict__ use, Kb8 k1, Kb8 k2,
              Mat3 R, V3 t, int *__restrict__ away) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    int v = 0;
    if (i < n && (!use || use[i])) {
        V3 r1, r2;
        epipolar_rays(k1, k2, uv1[2 * i], uv1[2 * i + 1], uv2[2 * i], uv2[2 * i + 1], r1, r2);   // :232-233
        const float tt[3] = {t.x, t.y, t.z};
        v = camera_vote(R.m, tt, r1, r2);
    }
    const unsigned long long pos = __ballot(v > 0), neg = __ballot(v < 0);
    const int d = __popcll(pos) - __popcll(neg);
    if ((threadIdx.x & 63) == 0 && d) atomicAdd(away, d);
}

}  // namespace dev

using namespace dev;

namespace {
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// decomposeE (:264-279) and the choice of Rgood (:253) in fp64 from the float E: R [9] row-major and the
// starting t (the unit left null vector of E, its component of largest magnitude positive), as floats.
// false: E has no two non-zero singular values
bool decompose_essential(const float *Ef, float *R, float *t) {
    double e[9], lam[3], V[9];
    for (int k = 0; k < 9; k++) e[k] = (double)Ef[k];
    gram_eigen(e, lam, V);
    if (!(lam[1] > 0.0) || !(lam[0] <= 1.7976931348623157e308)) return false;
    const double s1 = std::sqrt(lam[0]), s2 = std::sqrt(lam[1]);
    double u1[3], u2[3], u3[3];
    for (int a = 0; a < 3; a++) {
        u1[a] = (e[3 * a] * V[0] + e[3 * a + 1] * V[3] + e[3 * a + 2] * V[6]) / s1;
        u2[a] = (e[3 * a] * V[1] + e[3 * a + 1] * V[4] + e[3 * a + 2] * V[7]) / s2;
    }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    const double n3 = std::sqrt(u3[0] * u3[0] + u3[1] * u3[1] + u3[2] * u3[2]);
    if (!(n3 > 0.0)) return false;
    for (int a = 0; a < 3; a++) u3[a] = u3[a] / n3;
    // U W V^T = u2 v1^T - u1 v2^T + u3 v3^T (R2, :274) and U W^T V^T = -u2 v1^T + u1 v2^T + u3 v3^T (R1, :270)
    double R1[9], R2[9];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const double w = u2[a] * V[3 * b] - u1[a] * V[3 * b + 1], z = u3[a] * V[3 * b + 2];
            R2[3 * a + b] = w + z;
            R1[3 * a + b] = -w + z;
        }
    auto det = [](const double *m) {
        return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    };
    if (det(R1) < 0)
        for (double &v : R1) v = -v;
    if (det(R2) < 0)
        for (double &v : R2) v = -v;
    const double *Rg = (R2[0] + R2[4] + R2[8] > R1[0] + R1[4] + R1[8]) ? R2 : R1;   // :253
    for (int k = 0; k < 9; k++) R[k] = (float)Rg[k];
    double big = 0.0, lead = 1.0;
    for (int a = 0; a < 3; a++)
        if (std::fabs(u3[a]) > big) { big = std::fabs(u3[a]); lead = u3[a]; }
    for (int a = 0; a < 3; a++) t[a] = (float)(lead < 0 ? -u3[a] : u3[a]);
    return true;
}
}  // namespace

int find_essential_ransac(int device, hipStream_t st, int32_t n, const float *uv1, const float *uv2, const float *kb8_1,
                          const float *kb8_2, int32_t n_hyp, const int32_t *samples, float epipolar_th, float *E_best,
                          uint8_t *inlier, float *err_out, int32_t *scores, float *E_all, uint8_t *degenerate,
                          deftri_essential_report *report, std::string &err) {
    const auto t0 = std::chrono::steady_clock::now();
    const size_t N = (size_t)n, H = (size_t)n_hyp;
    for (size_t k = 0; k < 8 * H; k++)
        if (samples[k] < 0 || samples[k] >= n) {
            err = "find_essential_ransac: hypothesis " + std::to_string(k / 8) + " samples match " + std::to_string(samples[k]) +
                  ", outside [0, n = " + std::to_string(n) + ")";
            return DEFTRI_E_ARG;
        }
    Kb8 k1, k2;
    std::memcpy(k1.k, kb8_1, sizeof(k1.k));
    std::memcpy(k2.k, kb8_2, sizeof(k2.k));
    deftri_essential_report rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.n_matches = n;
    rep.n_hypotheses = n_hyp;

    if (device < 0) {
        std::vector<float> rays(6 * N), Eall(9 * H);
        std::vector<int32_t> sc(H, 0);
        std::vector<uint8_t> deg(H, 0);
        for (size_t i = 0; i < N; i++) {
            V3 r1, r2;
            epipolar_rays(k1, k2, uv1[2 * i], uv1[2 * i + 1], uv2[2 * i], uv2[2 * i + 1], r1, r2);
            rays[i] = r1.x; rays[N + i] = r1.y; rays[2 * N + i] = r1.z;
            rays[3 * N + i] = r2.x; rays[4 * N + i] = r2.y; rays[5 * N + i] = r2.z;
        }
        rep.ms_rays = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        double work[WORK];
        for (size_t h = 0; h < H; h++) {
            deg[h] = essential_model(rays.data(), n, samples + 8 * h, work, 1, &Eall[9 * h]) ? 0 : 1;
            rep.n_degenerate += deg[h];
        }
        rep.ms_models = ms_since(t1);
        const auto t2 = std::chrono::steady_clock::now();
        std::vector<V3> r2n(N);
        for (size_t i = 0; i < N; i++) r2n[i] = eigen_normalized(v3(rays[3 * N + i], rays[4 * N + i], rays[5 * N + i]));
        int best = -1, best_score = 0;
        for (size_t h = 0; h < H; h++) {
            if (deg[h]) continue;
            int s = 0;
            for (size_t i = 0; i < N; i++)
                if (epipolar_score(&Eall[9 * h], v3(rays[i], rays[N + i], rays[2 * N + i]), r2n[i]) < epipolar_th) s++;
            sc[h] = s;
            if (s > best_score) { best_score = s; best = (int)h; }      // :167
        }
        for (int k = 0; k < 9; k++) E_best[k] = best >= 0 ? Eall[9 * (size_t)best + k] : 0.0f;
        for (size_t i = 0; i < N; i++) {
            const float e = best >= 0 ? epipolar_score(E_best, v3(rays[i], rays[N + i], rays[2 * N + i]), r2n[i])
                                      : __builtin_nanf("");
            inlier[i] = (best >= 0 && e < epipolar_th) ? 1 : 0;
            if (err_out) err_out[i] = e;
        }
        rep.ms_score = ms_since(t2);
        if (scores) std::memcpy(scores, sc.data(), 4 * H);
        if (E_all) std::memcpy(E_all, Eall.data(), 36 * H);
        if (degenerate) std::memcpy(degenerate, deg.data(), H);
        rep.best = best;
        rep.best_score = best_score;
        rep.ms_total = ms_since(t0);
        if (report) *report = rep;
        return 0;
    }

    hipSetDevice(device);
    // the upload: uv1, uv2, samples; the download: head, err, scores, E_all, degenerate, inlier
    const size_t in_uv2 = align16(8 * N), in_samples = in_uv2 + align16(8 * N), in_bytes = in_samples + 32 * H;
    const size_t out_err = align16(sizeof(RansacHead)), out_scores = out_err + align16(4 * N), out_E = out_scores + align16(4 * H);
    const size_t out_deg = out_E + align16(36 * H), out_inl = out_deg + align16(H), out_bytes = out_inl + N;
    std::vector<char> in(in_bytes, 0), out(out_bytes);
    std::memcpy(in.data(), uv1, 8 * N);
    std::memcpy(in.data() + in_uv2, uv2, 8 * N);
    std::memcpy(in.data() + in_samples, samples, 32 * H);
    DevArena A;
    char *d_in, *d_out;
    float *d_rays;
    A.in(&d_in, in.data(), in_bytes); A.add(&d_out, out_bytes); A.add(&d_rays, 6 * N);
    if (!A.commit(st)) {
        err = "find_essential_ransac: allocation failed";
        return DEFTRI_E_HIP;
    }
    hipEvent_t ev[4];
    for (hipEvent_t &e : ev)
        if (hipEventCreate(&e) != hipSuccess) {
            err = "find_essential_ransac: hipEventCreate failed";
            return DEFTRI_E_HIP;
        }
    const float *d_uv1 = (const float *)d_in, *d_uv2 = (const float *)(d_in + in_uv2);
    const int *d_samples = (const int *)(d_in + in_samples);
    RansacHead *d_head = (RansacHead *)d_out;
    float *d_err = (float *)(d_out + out_err), *d_E = (float *)(d_out + out_E);
    int *d_scores = (int *)(d_out + out_scores);
    uint8_t *d_deg = (uint8_t *)(d_out + out_deg), *d_inl = (uint8_t *)(d_out + out_inl);
    hipMemsetAsync(d_out, 0, out_bytes, st);                 // the scores and n_degenerate start at 0
    const unsigned nb = (unsigned)((N + 255) / 256);
    hipEventRecord(ev[0], st);
    hipLaunchKernelGGL(dev::k_rays, dim3(nb), dim3(256), 0, st, n, d_uv1, d_uv2, k1, k2, d_rays);
    hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(dev::k_essential_models, dim3((unsigned)((H + MODEL_THREADS - 1) / MODEL_THREADS)), dim3(MODEL_THREADS), 0, st,
                       n, n_hyp, d_rays, d_samples, d_E, d_deg, &d_head->n_degenerate);
    hipEventRecord(ev[2], st);
    hipLaunchKernelGGL(dev::k_score, dim3(nb, (unsigned)((H + TILE_H - 1) / TILE_H)), dim3(256), 0, st, n, n_hyp, d_rays, d_E, d_deg,
                       epipolar_th, d_scores);
    hipLaunchKernelGGL(dev::k_best, dim3(1), dim3(256), 0, st, n, n_hyp, d_rays, d_E, d_scores, epipolar_th, d_head, d_inl, d_err);
    hipEventRecord(ev[3], st);
    hipMemcpyAsync(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    float ms[3] = {0.0f, 0.0f, 0.0f};
    if (e == hipSuccess)
        for (int k = 0; k < 3; k++) hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
    for (hipEvent_t &x : ev) hipEventDestroy(x);
    if (e != hipSuccess) return hip_fail(err, "find_essential_ransac", e);
    RansacHead head;
    std::memcpy(&head, out.data(), sizeof(head));
    std::memcpy(E_best, head.E_best, sizeof(head.E_best));
    std::memcpy(inlier, out.data() + out_inl, N);
    if (err_out) std::memcpy(err_out, out.data() + out_err, 4 * N);
    if (scores) std::memcpy(scores, out.data() + out_scores, 4 * H);
    if (E_all) std::memcpy(E_all, out.data() + out_E, 36 * H);
    if (degenerate) std::memcpy(degenerate, out.data() + out_deg, H);
    rep.n_degenerate = head.n_degenerate;
    rep.best = head.best;
    rep.best_score = head.best_score;
    rep.round_trips = 1;
    rep.ms_rays = ms[0];
    rep.ms_models = ms[1];
    rep.ms_score = ms[2];
    rep.ms_total = ms_since(t0);
    if (report) *report = rep;
    return 0;
}

int reconstruct_cameras(int device, hipStream_t st, int32_t n, const float *uv1, const float *uv2, const float *kb8_1,
                        const float *kb8_2, const uint8_t *use, const float *E, float *T2w, int32_t *away, std::string &err) {
    float R[9], t[3];
    if (!decompose_essential(E, R, t)) {
        err = "reconstruct_cameras: E has fewer than two non-zero singular values (or is not finite)";
        return DEFTRI_E_ARG;
    }
    Kb8 k1, k2;
    std::memcpy(k1.k, kb8_1, sizeof(k1.k));
    std::memcpy(k2.k, kb8_2, sizeof(k2.k));
    int vote = 0;
    const size_t N = (size_t)n;
    if (device < 0 || n == 0) {
        for (size_t i = 0; i < N; i++) {
            if (use && !use[i]) continue;
            V3 r1, r2;
            epipolar_rays(k1, k2, uv1[2 * i], uv1[2 * i + 1], uv2[2 * i], uv2[2 * i + 1], r1, r2);
            vote += camera_vote(R, t, r1, r2);
        }
    } else {
        hipSetDevice(device);
        const size_t in_uv2 = align16(8 * N), in_use = in_uv2 + align16(8 * N), in_bytes = in_use + N;
        std::vector<char> in(in_bytes, 0);
        std::memcpy(in.data(), uv1, 8 * N);
        std::memcpy(in.data() + in_uv2, uv2, 8 * N);
        if (use) std::memcpy(in.data() + in_use, use, N);
        DevArena A;
        char *d_in;
        int *d_away;
        A.in(&d_in, in.data(), in_bytes); A.add(&d_away, 1);
        if (!A.commit(st)) {
            err = "reconstruct_cameras: allocation failed";
            return DEFTRI_E_HIP;
        }
        Mat3 Rm;
        std::memcpy(Rm.m, R, sizeof(Rm.m));
        hipMemsetAsync(d_away, 0, sizeof(int), st);
        hipLaunchKernelGGL(dev::k_camera_vote, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, n, (const float *)d_in,
                           (const float *)(d_in + in_uv2), use ? (const uint8_t *)(d_in + in_use) : nullptr, k1, k2, Rm,
                           v3(t[0], t[1], t[2]), d_away);
        hipMemcpyAsync(&vote, d_away, sizeof(int), hipMemcpyDeviceToHost, st);
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(err, "reconstruct_cameras", e);
    }
    *away = vote;
    const float sgn = vote < 0 ? -1.0f : 1.0f;                // signbit(away) (:259)
    for (int a = 0; a < 3; a++) {
        T2w[4 * a] = R[3 * a]; T2w[4 * a + 1] = R[3 * a + 1]; T2w[4 * a + 2] = R[3 * a + 2];
        T2w[4 * a + 3] = sgn * t[a];
    }
    return 0;
}

}  // namespace deftri
