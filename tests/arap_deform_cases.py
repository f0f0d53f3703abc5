"""The cases of deftri_arap_deform that the host-only tests (test_arap_deform.py) and the device tests
(test_arap_deform_gpu.py) share: the seeded meshes, the LU references (computed once per case) and the checks, each
taking the context under test."""
import copy
import functools

import numpy as np

import arap_deform_ref as ref
from deftri import sim

CG_TOL = 1e-12          # the library's default relative residual


@functools.lru_cache(maxsize=None)
def mesh(n):
    v, tris = ref.seeded_mesh(n)
    v.setflags(write=False)
    tris.setflags(write=False)
    return v, tris


@functools.lru_cache(maxsize=None)
def four_handle_reference(n, energy, iters):
    """(ids, positions, reference p, reference energies, cond(A)); cond from the dense reduced matrix."""
    v, tris = mesh(n)
    ids, pos = ref.four_handles(v)
    p, en = ref.deform(v, tris, ids, pos, iters, energy)
    cond = float(np.linalg.cond(ref.reduced_matrix(v, tris, ids, pos)))
    for a in (ids, pos, p, en):
        a.setflags(write=False)
    return ids, pos, p, en, cond


def position_bound(cond, p):
    """10 cond(A) cg_tol max|p|: the textbook bound of one solve's error, times 10 for the carry-over across iterations."""
    return 10.0 * cond * CG_TOL * float(np.abs(p).max())


def check_four_handles(ctx, n, energy, iters=20):
    v, tris = mesh(n)
    ids, pos, p_ref, en_ref, cond = four_handle_reference(n, energy, iters)
    p, en, rep = ctx.arap_deform(v, tris, ids, pos, max_iter=iters, energy=energy)
    dist = float(np.abs(p - p_ref).max())
    bound = position_bound(cond, p_ref)
    rel = float(np.abs(en / en_ref - 1.0).max())
    print(f"arap_deform n={n} {energy}: max|p - p_LU| {dist:.3e} (bound {bound:.3e}, cond {cond:.1f}), energies rel {rel:.3e}, "
          f"E {en[0]:.6g} -> {en[-1]:.6g}, CG iterations {rep['cg_iterations']}")
    assert dist <= bound, (dist, bound)
    assert np.abs(p - p_ref).max() < 1e-2            # a wrong weight, transpose or sign moves points by more
    assert rel <= 1e-8, rel
    if energy == "spokes":
        assert np.all(np.diff(en) <= 0.0), en
    assert rep["iterations"] == iters and rep["n_constraints"] == 4 and rep["n_free"] == n - 4
    assert rep["cg_unconverged_steps"] == 0
    assert rep["energy_first"] == en[0] and rep["energy_last"] == en[-1]
    return p, en, rep


@functools.lru_cache(maxsize=None)
def single_constraint_cond(n):
    v, tris = mesh(n)
    return float(np.linalg.cond(ref.reduced_matrix(v, tris, np.zeros(10, np.int32), v)))


def check_reference_arguments(ctx, n):
    """Ten zero ids and all n positions as constraint positions: vertex 0 alone pinned to cpos[9], a translation."""
    v, tris = mesh(n)
    cpos = v + np.array([0.3, -0.2, 0.1]) + 0.05 * np.sin(np.arange(3 * n)).reshape(n, 3)
    cid = np.zeros(10, np.int32)
    p, en, rep = ctx.arap_deform(v, tris, cid, cpos, max_iter=20)
    want = v + (cpos[9] - v[0])
    bound = position_bound(single_constraint_cond(n), want)
    dist = float(np.abs(p - want).max())
    print(f"arap_deform n={n} reference arguments: max|p - translation| {dist:.3e} (bound {bound:.3e})")
    assert dist <= bound, (dist, bound)
    assert rep["n_constraints"] == 1 and rep["n_free"] == n - 1
    _, _, first = ctx.arap_deform(v, tris, cid, cpos, max_iter=1)
    assert first["cg_iterations"] > 0
    assert rep["cg_iterations"] == first["cg_iterations"]      # iterations 2 .. 20 start converged
    return p


def two_view_map():
    m, _ = sim.simulate_two_view(n=120)
    return m


@functools.lru_cache(maxsize=None)
def _map_reference():
    m = two_view_map()
    ref.open3d_map(m)
    return m


def positions(m, kid):
    return np.array([mp.position for mp in m.keyframes[kid].map_points if mp is not None], np.float32)


def check_map_entry(ctx, prepare=None):
    """Keyframe 1 (the later one in map order) bit-unchanged, keyframe 2 within one fp32 ulp of the reference."""
    m0 = two_view_map()
    m = copy.deepcopy(m0)
    if prepare:
        prepare(ctx)
    rep = ctx.arap_open3d_optimization(m)
    want = _map_reference()
    order = m.kf_order()
    kf2, kf1 = order[0], order[1]
    assert np.array_equal(positions(m, kf1), positions(m0, kf1))
    got, exp = positions(m, kf2), positions(want, kf2)
    ulp = np.spacing(np.abs(exp))
    worst = float((np.abs(got - exp) / ulp).max())
    print(f"arapOpen3DOptimization: keyframe 2 within {worst:.1f} ulp of the reference, {int((got != exp).sum())} of {got.size} differ")
    assert worst <= 1.0, worst
    assert not np.array_equal(got, positions(m0, kf2))
    assert rep["iterations"] == 500 and rep["n_constraints"] == 1
    return m, rep
