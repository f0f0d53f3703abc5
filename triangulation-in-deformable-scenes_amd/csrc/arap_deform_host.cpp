// arap_deform_host.cpp — as-rigid-as-possible mesh deformation (arap_deform.h): the call's set-up (adjacency,
// cot weights, constraint table, the component rule), the host path in plain loops, and the reference's
// arapOpen3DOptimization (g2oBundleAdjustment.cc:1010-1104) over the map view.
#include "arap_deform.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>
#include <unordered_map>

namespace deftri {
namespace arap {

namespace {
double ms_since(std::chrono::steady_clock::time_point a) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
}
int find_root(std::vector<int32_t> &parent, int x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
}
}  // namespace

int build_system(int32_t n, const double *vertices, int32_t n_tris, const int32_t *tris, int32_t n_cid, const int32_t *cid,
                 int32_t n_cpos, const double *cpos, const deftri_arap_deform_params *prm, System &S, std::string &err) {
    if (n < 3) { err = "arap_deform: fewer than 3 vertices"; return DEFTRI_E_ARG; }
    if (!vertices || n_tris < 0 || (n_tris > 0 && !tris)) { err = "arap_deform: null mesh array"; return DEFTRI_E_ARG; }
    S.max_iter = prm ? prm->max_iter : 50;
    S.energy = prm ? prm->energy : 0;
    S.alpha = prm ? prm->smoothed_alpha : 0.01;
    S.tol = prm && prm->cg_tol > 0 ? prm->cg_tol : 1e-12;
    S.cg_max = prm && prm->cg_max_iterations > 0 ? prm->cg_max_iterations : (int)std::min<int64_t>(10 * (int64_t)n + 100, INT32_MAX);
    if (S.max_iter < 0) { err = "arap_deform: max_iter < 0"; return DEFTRI_E_ARG; }
    if (S.energy != 0 && S.energy != 1) { err = "arap_deform: energy is 0 (Spokes) or 1 (Smoothed)"; return DEFTRI_E_ARG; }
    for (int64_t k = 0; k < 3 * (int64_t)n_tris; k++)
        if (tris[k] < 0 || tris[k] >= n) { err = "arap_deform: triangle " + std::to_string(k / 3) + " has a vertex out of range"; return DEFTRI_E_ARG; }
    const int m = std::min(n_cid, n_cpos);
    if (m <= 0) { err = "arap_deform: no effective constraint (min(n_cid, n_cpos) is 0)"; return DEFTRI_E_ARG; }
    if (!cid || !cpos) { err = "arap_deform: null constraint array"; return DEFTRI_E_ARG; }
    for (int k = 0; k < m; k++)
        if (cid[k] < 0 || cid[k] >= n) { err = "arap_deform: constraint " + std::to_string(k) + " names a vertex out of range"; return DEFTRI_E_ARG; }
    S.n = n;
    S.ntri = n_tris;
    S.v.assign(vertices, vertices + 3 * (size_t)n);
    S.tris.assign(tris, tris + 3 * (size_t)n_tris);
    S.con.assign(n, 0);
    S.cval.assign(3 * (size_t)n, 0.0);
    for (int k = 0; k < m; k++) {                       // a repeated id keeps its last position
        S.con[cid[k]] = 1;
        for (int c = 0; c < 3; c++) S.cval[3 * (size_t)cid[k] + c] = cpos[3 * (size_t)k + c];
    }
    S.n_con = (int)std::count(S.con.begin(), S.con.end(), 1);
    S.n_free = n - S.n_con;
    // adjacency (ComputeAdjacencyList): sorted, unique rows
    std::vector<int32_t> cnt(n + 1, 0);
    for (int64_t k = 0; k < 3 * (int64_t)n_tris; k++) cnt[tris[k] + 1] += 2;
    for (int i = 0; i < n; i++) cnt[i + 1] += cnt[i];
    std::vector<int32_t> tmp(cnt[n]), fill(cnt.begin(), cnt.end() - 1);
    for (int t = 0; t < n_tris; t++) {
        const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
        tmp[fill[a]++] = b; tmp[fill[a]++] = c;
        tmp[fill[b]++] = a; tmp[fill[b]++] = c;
        tmp[fill[c]++] = a; tmp[fill[c]++] = b;
    }
    S.off.assign(n + 1, 0);
    S.adj.resize(tmp.size());
    for (int i = 0; i < n; i++) {
        int32_t *b = tmp.data() + cnt[i], *e = tmp.data() + cnt[i + 1];
        std::sort(b, e);
        e = std::unique(b, e);
        e = std::remove(b, e, i);                       // a degenerate triangle's repeated vertex is no neighbour
        std::copy(b, e, S.adj.data() + S.off[i]);
        S.off[i + 1] = S.off[i] + (int32_t)(e - b);
    }
    S.adj.resize(S.off[n]);
    auto find = [&](int i, int j) -> int64_t {
        const int32_t *b = S.adj.data() + S.off[i], *e = S.adj.data() + S.off[i + 1];
        const int32_t *p = std::lower_bound(b, e, j);
        return (p != e && *p == j) ? (int64_t)(p - S.adj.data()) : -1;
    };
    // ComputeEdgeWeightsCot(mesh, 0): per edge (lo, hi) the mean of cot_term over its opposite vertices, clamped at 0
    std::vector<double> sum(S.adj.size(), 0.0);
    std::vector<int32_t> num(S.adj.size(), 0);
    for (int t = 0; t < n_tris; t++) {
        const int v3[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
        for (int k = 0; k < 3; k++) {
            const int e0 = std::min(v3[k], v3[(k + 1) % 3]), e1 = std::max(v3[k], v3[(k + 1) % 3]), v2 = v3[(k + 2) % 3];
            if (e0 == e1) continue;
            const int64_t at = find(e0, e1);
            sum[at] += cot_term(&S.v[3 * (size_t)e0], &S.v[3 * (size_t)e1], &S.v[3 * (size_t)v2]);
            num[at]++;
        }
    }
    S.w.assign(S.adj.size(), 0.0);
    S.zero_edges = 0;
    std::vector<int32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0);
    for (int i = 0; i < n; i++)
        for (int32_t k = S.off[i]; k < S.off[i + 1]; k++) {
            const int j = S.adj[k];
            if (j < i) continue;
            double wt = cot_weight(sum[k], num[k]);
            if (!(wt > 0.0) && wt == wt) wt = 0.0;     // -0 -> 0; a NaN weight (a degenerate triangle) stays and fails below
            S.w[k] = S.w[find(j, i)] = wt;
            if (wt > 0.0) {
                const int a = find_root(parent, i), b = find_root(parent, j);
                if (a != b) parent[std::max(a, b)] = std::min(a, b);
            } else {
                S.zero_edges++;
            }
        }
    S.diag.assign(n, 0.0);
    for (int i = 0; i < n; i++)
        for (int32_t k = S.off[i]; k < S.off[i + 1]; k++) S.diag[i] += S.w[k];
    for (int i = 0; i < n; i++)
        if (!std::isfinite(S.diag[i])) { err = "arap_deform: vertex " + std::to_string(i) + " has a non-finite edge weight (a degenerate triangle)"; return DEFTRI_E_GRAPH; }
    // the component rule: every component of the positive-weight edges holds a constrained vertex
    std::vector<uint8_t> held(n, 0);
    for (int i = 0; i < n; i++)
        if (S.con[i]) held[find_root(parent, i)] = 1;
    for (int i = 0; i < n; i++)
        if (!held[find_root(parent, i)]) {
            err = "arap_deform: vertex " + std::to_string(i) + " lies in a component of the positive-weight edges without a constrained vertex (the system matrix is singular)";
            return DEFTRI_E_GRAPH;
        }
    return 0;
}

int run_host(const System &S, double *out, double *energies, deftri_arap_deform_report *rep, std::string &err) {
    const int n = S.n;
    const int32_t *off = S.off.data(), *adj = S.adj.data(), *con = S.con.data();
    const double *w = S.w.data(), *v = S.v.data(), *diag = S.diag.data(), *cval = S.cval.data();
    double area = 0;
    for (int t = 0; t < S.ntri; t++)
        area += tri_area(&v[3 * (size_t)S.tris[3 * t]], &v[3 * (size_t)S.tris[3 * t + 1]], &v[3 * (size_t)S.tris[3 * t + 2]]);
    rep->area = area;
    std::vector<double> p(S.v), R(9 * (size_t)n), Rold(9 * (size_t)n), r(3 * (size_t)n), z(r), d(r), q(r), en(S.max_iter);
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 9; k++) R[9 * (size_t)i + k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int it = 0; it < S.max_iter; it++) {
        const auto t0 = std::chrono::steady_clock::now();
        const double smooth_c = (S.energy == 1 && it > 0) ? 4.0 * S.alpha * area : 0.0;
        if (S.energy == 1) R.swap(Rold);
        for (int i = 0; i < n; i++)
            if (!(local_rotation(i, off, adj, w, v, p.data(), smooth_c, Rold.data(), &R[9 * (size_t)i]) > 0.0)) {
                err = "arap_deform: det R <= 0 at vertex " + std::to_string(i) + ", iteration " + std::to_string(it + 1);
                return DEFTRI_E_NUMERIC;
            }
        rep->ms_local += ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        // global step: PCG on the reduced system, the three columns at once, from the previous iterate
        double bb[3] = {0, 0, 0}, rr[3] = {0, 0, 0}, rz[3] = {0, 0, 0};
        for (int i = 0; i < n; i++) {
            if (con[i]) {
                for (int c = 0; c < 3; c++) { p[3 * i + c] = cval[3 * i + c]; r[3 * i + c] = z[3 * i + c] = d[3 * i + c] = 0.0; }
                continue;
            }
            double b[3], Ap[3];
            rhs_row(i, off, adj, w, diag, con, cval, v, p.data(), R.data(), b, Ap);
            for (int c = 0; c < 3; c++) {
                const double ri = b[c] - Ap[c], zi = ri / diag[i];
                r[3 * i + c] = ri; z[3 * i + c] = zi; d[3 * i + c] = zi;
                bb[c] += b[c] * b[c]; rr[c] += ri * ri; rz[c] += ri * zi;
            }
        }
        double thr[3];
        bool conv[3];
        for (int c = 0; c < 3; c++) { thr[c] = S.tol * S.tol * bb[c]; conv[c] = rr[c] <= thr[c]; }
        int iters[3] = {0, 0, 0};
        for (int k = 0; k < S.cg_max && !(conv[0] && conv[1] && conv[2]); k++) {
            double dq[3] = {0, 0, 0};
            for (int i = 0; i < n; i++) {
                if (con[i]) continue;
                spmv_row(i, off, adj, w, diag, d.data(), &q[3 * (size_t)i]);
                for (int c = 0; c < 3; c++) dq[c] += d[3 * i + c] * q[3 * i + c];
            }
            double a[3], rrn[3] = {0, 0, 0}, rzn[3] = {0, 0, 0};
            for (int c = 0; c < 3; c++) { a[c] = conv[c] ? 0.0 : rz[c] / dq[c]; if (!conv[c]) iters[c]++; }
            for (int i = 0; i < n; i++) {
                if (con[i]) continue;
                for (int c = 0; c < 3; c++) {
                    if (!conv[c]) {
                        p[3 * i + c] += a[c] * d[3 * i + c];
                        r[3 * i + c] -= a[c] * q[3 * i + c];
                        z[3 * i + c] = r[3 * i + c] / diag[i];
                    }
                    rrn[c] += r[3 * i + c] * r[3 * i + c];
                    rzn[c] += r[3 * i + c] * z[3 * i + c];
                }
            }
            for (int c = 0; c < 3; c++) {
                if (conv[c]) continue;
                conv[c] = rrn[c] <= thr[c];
                if (!conv[c]) {
                    const double beta = rzn[c] / rz[c];
                    for (int i = 0; i < n; i++)
                        if (!con[i]) d[3 * i + c] = z[3 * i + c] + beta * d[3 * i + c];
                }
                rz[c] = rzn[c];
            }
        }
        const int mx = std::max(iters[0], std::max(iters[1], iters[2]));
        rep->cg_iterations += (int64_t)iters[0] + iters[1] + iters[2];
        rep->cg_max_in_step = std::max(rep->cg_max_in_step, mx);
        rep->ms_global += ms_since(t1);
        rep->iterations = it + 1;
        if (!(conv[0] && conv[1] && conv[2])) {
            rep->cg_unconverged_steps++;
            err = "arap_deform: the global step of iteration " + std::to_string(it + 1) + " did not reach cg_tol within " +
                  std::to_string(S.cg_max) + " CG iterations";
            return DEFTRI_E_NUMERIC;
        }
        double E = 0, Ereg = 0;
        for (int i = 0; i < n; i++) {
            double ef, er;
            energy_vertex(i, off, adj, w, v, p.data(), R.data(), S.energy == 1, ef, er);
            E += ef;
            Ereg += er;
        }
        if (S.energy == 1) E += S.alpha * area * Ereg;
        if (!std::isfinite(E)) { err = "arap_deform: non-finite iterate at iteration " + std::to_string(it + 1); return DEFTRI_E_NUMERIC; }
        en[it] = E;
    }
    for (size_t k = 0; k < p.size(); k++)
        if (!std::isfinite(p[k])) { err = "arap_deform: non-finite iterate"; return DEFTRI_E_NUMERIC; }
    if (S.max_iter > 0) { rep->energy_first = en[0]; rep->energy_last = en[S.max_iter - 1]; }
    std::copy(p.begin(), p.end(), out);
    if (energies) std::copy(en.begin(), en.end(), energies);
    return 0;
}

int deform(int device, hipStream_t st, int32_t n, const double *vertices, int32_t n_tris, const int32_t *tris, int32_t n_cid,
           const int32_t *cid, int32_t n_cpos, const double *cpos, const deftri_arap_deform_params *prm, double *out,
           double *energies, deftri_arap_deform_report *rep, std::string &err) {
    const auto t0 = std::chrono::steady_clock::now();
    deftri_arap_deform_report local{};
    deftri_arap_deform_report &R = rep ? *rep : local;
    R = deftri_arap_deform_report{};
    if (!out) { err = "arap_deform: null output"; return DEFTRI_E_ARG; }
    System S;
    int rc = build_system(n, vertices, n_tris, tris, n_cid, cid, n_cpos, cpos, prm, S, err);
    if (rc) return rc;
    R.n_constraints = S.n_con;
    R.n_free = S.n_free;
    R.zero_weight_edges = S.zero_edges;
    R.on_device = device >= 0 ? 1 : 0;
    rc = device >= 0 ? run_device(device, st, S, out, energies, &R, err) : run_host(S, out, energies, &R, err);
    R.ms_total = ms_since(t0);
    return rc;
}

}  // namespace arap

int arap_open3d_map(int device, hipStream_t st, deftri_map &map, int pair_window, const MeshSource *mesh_src,
                    deftri_arap_deform_report *rep, std::string &err) {
    const int K = map.n_keyframes;
    if (K < 0 || (K > 0 && !map.keyframes)) { err = "arapOpen3DOptimization: null keyframes"; return DEFTRI_E_ARG; }
    // the MapPoints as objects: working copies of every keyframe's positions, and every slot of an id
    std::vector<std::vector<float>> pos(K);
    std::unordered_map<int64_t, std::vector<std::pair<int32_t, int32_t>>> slots_of;
    for (int k = 0; k < K; k++) {
        const deftri_keyframe &kf = map.keyframes[k];
        if (kf.n_slots < 0 || (kf.n_slots > 0 && (!kf.point_id || !kf.point_pos))) { err = "arapOpen3DOptimization: null slot arrays"; return DEFTRI_E_ARG; }
        pos[k].assign(kf.point_pos, kf.point_pos + 3 * (size_t)kf.n_slots);
        for (int s = 0; s < kf.n_slots; s++)
            if (kf.point_id[s] >= 0) slots_of[kf.point_id[s]].push_back({k, s});
    }
    auto set_position = [&](int64_t id, const float *p3) {      // MapPoint::setWorldPosition
        for (const auto &ks : slots_of[id])
            for (int c = 0; c < 3; c++) pos[ks.first][3 * (size_t)ks.second + c] = p3[c];
    };
    auto extract = [&](int k) {                                // extractPositions: the null slots dropped
        std::vector<double> out;
        const deftri_keyframe &kf = map.keyframes[k];
        for (int s = 0; s < kf.n_slots; s++)
            if (kf.point_id[s] >= 0)
                for (int c = 0; c < 3; c++) out.push_back((double)pos[k][3 * (size_t)s + c]);
        return out;
    };
    deftri_arap_deform_params prm{};
    prm.max_iter = 500;
    prm.energy = 0;
    prm.smoothed_alpha = 0.01;
    for (int a = 0; a < K; a++)
        for (int b = a + 1; b < K; b++) {
            if (pair_window > 0 && b - a > pair_window) continue;
            const deftri_keyframe &kf1 = map.keyframes[b], &kf2 = map.keyframes[a];   // pKF1 = k2->second, pKF2 = k1->second
            const std::vector<double> v1 = extract(b), v2 = extract(a);
            const int n1 = (int)v1.size() / 3, n2 = (int)v2.size() / 3;
            std::vector<int32_t> tris, pos_idx;
            if (!keyframe_mesh(v1, n1, mesh_src, tris, pos_idx, err)) return DEFTRI_E_GRAPH;
            std::vector<int32_t> inv(n1, -1);                  // invertedPosIndexes1: the later mesh vertex wins
            for (int v = 0; v < n1; v++) inv[pos_idx[v]] = v;
            const std::vector<int32_t> cid(10, 0);             // std::vector<int> constraint_vertex_indices(10)
            std::vector<double> deformed(3 * (size_t)n1);
            const int rc = arap::deform(device, st, n1, v1.data(), (int)tris.size() / 3, tris.data(), 10, cid.data(), n2, v2.data(),
                                        &prm, deformed.data(), nullptr, rep, err);
            if (rc) return rc;
            for (int mp = 0; mp < kf1.n_slots; mp++) {         // mpIndex: a slot index looked up as a position index
                if (mp >= n1 || inv[mp] < 0) continue;
                if (kf1.point_id[mp] < 0 || mp >= kf2.n_slots || kf2.point_id[mp] < 0) {
                    err = "arapOpen3DOptimization: slot " + std::to_string(mp) + " of keyframe " +
                          std::to_string(kf1.point_id[mp] < 0 ? kf1.id : kf2.id) + " is empty or past the end where the reference dereferences it";
                    return DEFTRI_E_ARG;
                }
                const int mv = inv[mp];
                const float p1[3] = {(float)v1[3 * (size_t)mv], (float)v1[3 * (size_t)mv + 1], (float)v1[3 * (size_t)mv + 2]};
                const float p2[3] = {(float)deformed[3 * (size_t)mv], (float)deformed[3 * (size_t)mv + 1], (float)deformed[3 * (size_t)mv + 2]};
                set_position(kf1.point_id[mp], p1);
                set_position(kf2.point_id[mp], p2);
            }
        }
    for (int k = 0; k < K; k++) std::copy(pos[k].begin(), pos[k].end(), map.keyframes[k].point_pos);
    return 0;
}

}  // namespace deftri
