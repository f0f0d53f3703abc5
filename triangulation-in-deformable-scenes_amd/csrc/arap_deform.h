// arap_deform.h — as-rigid-as-possible mesh deformation with handle constraints: the local/global
// iteration of Sorkine and Alexa as Open3D's TriangleMesh::DeformAsRigidAsPossible states it, restated
// (Open3D's source was not available and nothing here has been run against it).
//   local step   R_i = V diag(1, 1, det(V U^T)) U^T of S_i = sum_j w_ij (v_i - v_j)(p_i - p_j)^T
//   global step  L p = b, the constrained rows eliminated: A = L_ff is symmetric positive definite when
//                every component of the positive-weight edges holds a constrained vertex
// The per-vertex functions below are the arithmetic of both paths: the host loops (arap_deform_host.cpp) and
// the device kernels (arap_deform.hip).  Both files are built with FMA contraction off.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/deftri.h"
#include "graph_builder.h"
#include "procrustes.h"

namespace deftri {
namespace arap {

// One call's mesh and constraints as both paths read them (host arrays)
struct System {
    int n = 0, ntri = 0, max_iter = 0, energy = 0, cg_max = 0;
    double alpha = 0, tol = 0;
    std::vector<double> v;            // [3n] rest positions
    std::vector<int32_t> tris;        // [3 ntri]
    std::vector<int32_t> off, adj;    // CSR adjacency, rows sorted
    std::vector<double> w;            // per CSR entry: the cot weight, clamped at 0
    std::vector<double> diag;         // [n] sum_j w_ij
    std::vector<int32_t> con;         // [n] 1: constrained
    std::vector<double> cval;         // [3n] the constraint's position (rows with con)
    int n_con = 0, n_free = 0, zero_edges = 0;
};

// v, tris, constraints -> System: adjacency, weights, constraint table.  Returns 0, DEFTRI_E_ARG (err) or
// DEFTRI_E_GRAPH (a component of the positive-weight edges without a constrained vertex)
int build_system(int32_t n, const double *vertices, int32_t n_tris, const int32_t *tris, int32_t n_cid, const int32_t *cid,
                 int32_t n_cpos, const double *cpos, const deftri_arap_deform_params *prm, System &S, std::string &err);

// The iteration on the host / on the device: out [3n], energies [max_iter] (may be null), rep's counters
// and times.  out is written only when the call returns 0.
int run_host(const System &S, double *out, double *energies, deftri_arap_deform_report *rep, std::string &err);
int run_device(int device, hipStream_t st, const System &S, double *out, double *energies, deftri_arap_deform_report *rep,
               std::string &err);

// validation + build_system + the path the context has
int deform(int device, hipStream_t st, int32_t n, const double *vertices, int32_t n_tris, const int32_t *tris, int32_t n_cid,
           const int32_t *cid, int32_t n_cpos, const double *cpos, const deftri_arap_deform_params *prm, double *out,
           double *energies, deftri_arap_deform_report *rep, std::string &err);

// ---- per-vertex arithmetic ----------------------------------------------------------------------------

// the local step of vertex i: R [9] row-major.  smooth_c = 4 alpha area (Smoothed, from the second
// iteration on; Rold then holds the previous rotations), 0 otherwise.  Returns det R.
__host__ __device__ inline double local_rotation(int i, const int32_t *off, const int32_t *adj, const double *w, const double *v,
                                                 const double *p, double smooth_c, const double *Rold, double *R) {
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double Rs[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int32_t b = off[i], e = off[i + 1];
    for (int32_t k = b; k < e; k++) {
        const int j = adj[k];
        const double wt = w[k];
        double e1[3], e2[3];
        for (int c = 0; c < 3; c++) { e1[c] = v[3 * i + c] - v[3 * j + c]; e2[c] = p[3 * i + c] - p[3 * j + c]; }
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) S[3 * r + c] += wt * e1[r] * e2[c];
        if (smooth_c != 0.0)
            for (int q = 0; q < 9; q++) Rs[q] += Rold[9 * (size_t)j + q];
    }
    if (smooth_c != 0.0) {
        const double f = smooth_c / (double)(e - b);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) S[3 * r + c] = 2.0 * S[3 * r + c] + f * Rs[3 * c + r];
    }
    double U[9], sv[3], V[9], M[9];
    pr::jacobi_svd3(S, U, sv, V);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) M[3 * r + c] = V[3 * r] * U[3 * c] + V[3 * r + 1] * U[3 * c + 1] + V[3 * r + 2] * U[3 * c + 2];
    const double d = pr::det3(M);                        // D = diag(1, 1, det(V U^T))
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            R[3 * r + c] = V[3 * r] * U[3 * c] + V[3 * r + 1] * U[3 * c + 1] + d * (V[3 * r + 2] * U[3 * c + 2]);
    return pr::det3(R);
}

// the reduced system's right-hand side of a free vertex i: sum_j (w_ij / 2)(R_i + R_j)(v_i - v_j), a
// constrained neighbour adding w_ij c_j; and A p of the current iterate over the free neighbours
__host__ __device__ inline void rhs_row(int i, const int32_t *off, const int32_t *adj, const double *w, const double *diag,
                                        const int32_t *con, const double *cval, const double *v, const double *p,
                                        const double *R, double b[3], double Ap[3]) {
    const double *Ri = R + 9 * (size_t)i;
    for (int c = 0; c < 3; c++) { b[c] = 0.0; Ap[c] = diag[i] * p[3 * i + c]; }
    for (int32_t k = off[i]; k < off[i + 1]; k++) {
        const int j = adj[k];
        const double wt = w[k], h = 0.5 * wt;
        const double *Rj = R + 9 * (size_t)j;
        const double e[3] = {v[3 * i] - v[3 * j], v[3 * i + 1] - v[3 * j + 1], v[3 * i + 2] - v[3 * j + 2]};
        for (int r = 0; r < 3; r++)
            b[r] += h * ((Ri[3 * r] + Rj[3 * r]) * e[0] + (Ri[3 * r + 1] + Rj[3 * r + 1]) * e[1] + (Ri[3 * r + 2] + Rj[3 * r + 2]) * e[2]);
        if (con[j])
            for (int c = 0; c < 3; c++) b[c] += wt * cval[3 * j + c];
        else
            for (int c = 0; c < 3; c++) Ap[c] -= wt * p[3 * j + c];
    }
}

// A d of a free row over vectors whose constrained entries are zero
__host__ __device__ inline void spmv_row(int i, const int32_t *off, const int32_t *adj, const double *w, const double *diag,
                                         const double *d, double q[3]) {
    for (int c = 0; c < 3; c++) q[c] = diag[i] * d[3 * i + c];
    for (int32_t k = off[i]; k < off[i + 1]; k++) {
        const int j = adj[k];
        const double wt = w[k];
        for (int c = 0; c < 3; c++) q[c] -= wt * d[3 * j + c];
    }
}

// vertex i's share of the energy: sum_j w_ij |(p_i - p_j) - R_i (v_i - v_j)|^2 and, Smoothed, sum_j |R_i - R_j|_F^2
__host__ __device__ inline void energy_vertex(int i, const int32_t *off, const int32_t *adj, const double *w, const double *v,
                                              const double *p, const double *R, bool smoothed, double &e_fit, double &e_reg) {
    const double *Ri = R + 9 * (size_t)i;
    e_fit = 0.0;
    e_reg = 0.0;
    for (int32_t k = off[i]; k < off[i + 1]; k++) {
        const int j = adj[k];
        const double e[3] = {v[3 * i] - v[3 * j], v[3 * i + 1] - v[3 * j + 1], v[3 * i + 2] - v[3 * j + 2]};
        double s = 0.0;
        for (int r = 0; r < 3; r++) {
            const double d = (p[3 * i + r] - p[3 * j + r]) - (Ri[3 * r] * e[0] + Ri[3 * r + 1] * e[1] + Ri[3 * r + 2] * e[2]);
            s += d * d;
        }
        e_fit += w[k] * s;
        if (smoothed) {
            const double *Rj = R + 9 * (size_t)j;
            for (int q = 0; q < 9; q++) { const double d = Ri[q] - Rj[q]; e_reg += d * d; }
        }
    }
}

// a triangle's area
__host__ __device__ inline double tri_area(const double *p0, const double *p1, const double *p2) {
    const double x[3] = {p0[0] - p1[0], p0[1] - p1[1], p0[2] - p1[2]};
    const double y[3] = {p0[0] - p2[0], p0[1] - p2[1], p0[2] - p2[2]};
    const double cr[3] = {x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]};
    return 0.5 * sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
}

}  // namespace arap

// arapOpen3DOptimization(Map*) (g2oBundleAdjustment.cc:1010-1104) over the map view: every keyframe pair in
// map order, sequentially, on the positions the pairs before it wrote.  The map is written only when
// every pair succeeded.  mesh_src as build_arap_graph takes it; rep (may be null): the last pair's.
int arap_open3d_map(int device, hipStream_t st, deftri_map &map, int pair_window, const MeshSource *mesh_src,
                    deftri_arap_deform_report *rep, std::string &err);
}  // namespace deftri
