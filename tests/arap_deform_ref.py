"""Reference for deftri_arap_deform: Open3D's TriangleMesh::DeformAsRigidAsPossible restated in numpy, the
global step by the exact sparse LU (scipy.sparse.linalg.splu of the full system matrix, factored once) that
Open3D uses.  The mesh, the cot weights and the vector map are oracle.graph_ref's restatements.

  1. C[cid[k]] = cpos[k] for k < min(len(cid), len(cpos)); a repeated id keeps its last position
  2. w_ij = ComputeEdgeWeightsCot(mesh, 0): the mean over the edge's opposite vertices of a.b / |a x b|, clamped at 0
  3. L: unit rows for i in C, else L_ij = -w_ij, L_ii = sum_j w_ij
  4. p = v, R_i = I; max_iter times: S_i = sum_j w_ij (v_i - v_j)(p_i - p_j)^T (Smoothed, from the second iteration:
     2 S_i + (4 alpha area / nb_i)(sum_j R_old_j)^T), R_i = V diag(1, 1, det(V U^T)) U^T; b_i = C[i] or
     sum_j (w_ij / 2)(R_i + R_j)(v_i - v_j); L p = b; E = sum_i sum_j w_ij |(p_i - p_j) - R_i (v_i - v_j)|^2
     (+ alpha area sum_i sum_j |R_i - R_j|_F^2)
"""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import splu
from scipy.spatial import Delaunay

from oracle import graph_ref


def seeded_mesh(n, seed=3):
    """xy uniform in [-1, 1]^2, z = 2 + 0.1 N(0, 1), the Delaunay triangulation of xy."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    z = 2.0 + 0.1 * rng.standard_normal(n)
    v = np.c_[xy, z]
    tris = Delaunay(xy).simplices.astype(np.int32)
    return v, tris


def four_handles(v):
    """The vertices extreme in x + y and x - y, moved +0.5, -0.5, +0.5, -0.5 in z."""
    s, d = v[:, 0] + v[:, 1], v[:, 0] - v[:, 1]
    ids = np.array([np.argmax(s), np.argmin(s), np.argmax(d), np.argmin(d)], np.int32)
    pos = v[ids].copy()
    pos[:, 2] += np.array([0.5, -0.5, 0.5, -0.5])
    return ids, pos


def constraints(cid, cpos):
    C = {}
    for k in range(min(len(cid), len(cpos))):
        C[int(cid[k])] = np.asarray(cpos[k], np.float64)
    return C


def edges(v, tris):
    """Directed edges (I, J, W) of the adjacency, the neighbour counts and the surface area."""
    adj, w, area = graph_ref.mesh_structures(np.asarray(v, np.float64), np.asarray(tris))
    I, J, W = [], [], []
    for i, nb in enumerate(adj):
        for j in sorted(nb):
            I.append(i); J.append(j); W.append(w[(min(i, j), max(i, j))])
    return np.array(I, np.int64), np.array(J, np.int64), np.array(W), np.array([len(a) for a in adj]), area


def system_matrix(n, I, J, W, C):
    free = np.array([i not in C for i in range(n)])
    diag = np.zeros(n)
    np.add.at(diag, I, W)
    keep = free[I]
    rows = np.r_[I[keep], np.arange(n)]
    cols = np.r_[J[keep], np.arange(n)]
    vals = np.r_[-W[keep], np.where(free, diag, 1.0)]
    return sp.csc_matrix((vals, (rows, cols)), shape=(n, n)), free, diag


def reduced_matrix(v, tris, cid, cpos):
    """The dense reduced matrix A = L_ff (symmetric positive definite) of the free vertices."""
    n = len(v)
    I, J, W, _, _ = edges(v, tris)
    L, free, _ = system_matrix(n, I, J, W, constraints(cid, cpos))
    f = np.flatnonzero(free)
    return L.toarray()[np.ix_(f, f)]


def _rotations(S):
    U, s, Vt = np.linalg.svd(S)
    V = np.swapaxes(Vt, 1, 2)
    det = np.linalg.det(V @ np.swapaxes(U, 1, 2))
    D = np.zeros_like(S)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = det
    R = V @ D @ np.swapaxes(U, 1, 2)
    # a rank-deficient S_i (fewer than two independent weighted edges) leaves R_i to the SVD's own steps: Eigen's Jacobi
    for i in np.flatnonzero(s[:, 1] <= 1e-9 * np.maximum(s[:, 0], 1e-300)):
        Ue, _, Ve = graph_ref.eigen_jacobi_svd3(S[i])
        Ue, Ve = np.asarray(Ue), np.asarray(Ve)
        R[i] = Ve @ np.diag([1.0, 1.0, np.linalg.det(Ve @ Ue.T)]) @ Ue.T
    return R


def deform(v, tris, cid, cpos, max_iter=50, energy="spokes", smoothed_alpha=0.01):
    """Returns (p [n, 3], energies [max_iter])."""
    v = np.asarray(v, np.float64)
    n = len(v)
    C = constraints(cid, cpos)
    I, J, W, nb, area = edges(v, tris)
    L, free, _ = system_matrix(n, I, J, W, C)
    lu = splu(L)
    smoothed = energy.lower() == "smoothed"
    p = v.copy()
    R = np.tile(np.eye(3), (n, 1, 1))
    e1 = v[I] - v[J]
    cidx = np.array(sorted(C), np.int64)
    cval = np.array([C[i] for i in cidx])
    energies = np.zeros(max_iter)
    for it in range(max_iter):
        R_old = R
        e2 = p[I] - p[J]
        S = np.zeros((n, 3, 3))
        np.add.at(S, I, W[:, None, None] * e1[:, :, None] * e2[:, None, :])
        if smoothed and it > 0:
            Rs = np.zeros((n, 3, 3))
            np.add.at(Rs, I, R_old[J])
            S = 2.0 * S + (4.0 * smoothed_alpha * area / nb)[:, None, None] * np.swapaxes(Rs, 1, 2)
        R = _rotations(S)
        if (np.linalg.det(R) <= 0).any():
            raise ArithmeticError("det R <= 0")
        b = np.zeros((n, 3))
        np.add.at(b, I, 0.5 * W[:, None] * np.einsum("eij,ej->ei", R[I] + R[J], e1))
        b[cidx] = cval
        p = np.column_stack([lu.solve(b[:, c]) for c in range(3)])
        diff = (p[I] - p[J]) - np.einsum("eij,ej->ei", R[I], e1)
        E = float((W * (diff * diff).sum(1)).sum())
        if smoothed:
            dR = R[I] - R[J]
            E += smoothed_alpha * area * float((dR * dR).sum())
        energies[it] = E
    return p, energies


def open3d_map(m):
    """arapOpen3DOptimization (g2oBundleAdjustment.cc:1010-1104) on the Python map model, in place, with deform()."""
    order = m.kf_order()
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            kf1, kf2 = m.keyframes[order[b]], m.keyframes[order[a]]      # pKF1 = k2->second, pKF2 = k1->second
            v1 = np.array([mp.position for mp in kf1.map_points if mp is not None], np.float64).reshape(-1, 3)
            v2 = np.array([mp.position for mp in kf2.map_points if mp is not None], np.float64).reshape(-1, 3)
            tri, _ = graph_ref.delaunay_mesh(v1)
            pos_idx = graph_ref.create_vector_map(v1)
            inv = {}
            for k in range(len(v1)):
                inv[int(pos_idx[k])] = k
            out, _ = deform(v1, tri, np.zeros(10, np.int32), v2, max_iter=500, energy="spokes", smoothed_alpha=0.01)
            for mp_index in range(len(kf1.map_points)):
                if mp_index not in inv:
                    continue
                k = inv[mp_index]
                kf1.map_points[mp_index].position = v1[k].astype(np.float32)
                kf2.map_points[mp_index].position = out[k].astype(np.float32)
