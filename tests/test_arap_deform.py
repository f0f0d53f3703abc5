"""deftri_arap_deform and deftri_arap_open3d_optimization on a host-only context: Open3D's
DeformAsRigidAsPossible restated, held to the LU reference of tests/arap_deform_ref.py.  The device path runs the
same cases in tests/test_arap_deform_gpu.py."""
import copy
import ctypes as C

import numpy as np
import pytest

import arap_deform_cases as cases
import arap_deform_ref as ref
from deftri import _abi, capi, optimization
from deftri.settings import Settings

E_ARG, E_NUMERIC, E_GRAPH = -1, -4, -6


@pytest.fixture(scope="module")
def host():
    with capi.Context(-1) as c:
        yield c


@pytest.mark.parametrize("energy", ["spokes", "smoothed"])
@pytest.mark.parametrize("n", [65, 257])
def test_four_handles_against_the_lu_reference(host, n, energy):
    """Measured on the host path, max|p - p_LU| / bound: n = 65 2.0e-12 / 3.0e-9 (Spokes), 9.8e-13 / 3.0e-9
    (Smoothed); n = 257 6.6e-12 / 4.7e-8, 3.5e-12 / 4.6e-8.  Energies agree to 6e-12 relative."""
    _, _, rep = cases.check_four_handles(host, n, energy)
    assert rep["on_device"] == 0
    assert rep["zero_weight_edges"] == {65: 15, 257: 75}[n]      # the clamp at 0 is exercised


@pytest.mark.parametrize("n", [65, 257])
def test_the_references_own_arguments_translate_the_mesh(host, n):
    cases.check_reference_arguments(host, n)


def test_three_vertices_three_constraints(host):
    v, tris = cases.mesh(3)
    assert len(tris) == 1
    cpos = v[::-1] + 0.25
    p, en, rep = host.arap_deform(v, tris, [0, 1, 2], cpos, max_iter=5)
    assert np.array_equal(p, cpos)
    assert rep["n_free"] == 0 and rep["n_constraints"] == 3 and rep["cg_iterations"] == 0


def test_a_repeated_id_keeps_its_last_position_and_extra_ids_are_dropped(host):
    v, tris = cases.mesh(65)
    ids, pos = ref.four_handles(v)
    want, want_en, _ = host.arap_deform(v, tris, ids, pos, max_iter=5)
    # handle 0 named twice: the later position holds
    p, en, rep = host.arap_deform(v, tris, np.r_[ids[:1], ids], np.r_[pos[:1] + 7.0, pos], max_iter=5)
    assert rep["n_constraints"] == 4
    assert np.array_equal(p, want) and np.array_equal(en, want_en)
    # n_cid > n_cpos: the ids past the positions do not constrain anything
    p, en, rep = host.arap_deform(v, tris, np.r_[ids, [5, 6, 7]], pos, max_iter=5)
    assert rep["n_constraints"] == 4
    assert np.array_equal(p, want)
    # n_cpos > n_cid: the positions past the ids are not read
    p, _, rep = host.arap_deform(v, tris, ids[:3], pos, max_iter=5)
    assert rep["n_constraints"] == 3
    p_ref, _ = ref.deform(v, tris, ids[:3], pos, 5)
    assert np.abs(p - p_ref).max() < 1e-8


def _raw_call(ctx, v, tris, cid, cpos, max_iter=5, energy=0, out=None):
    v = np.ascontiguousarray(v, np.float64)
    tris = np.ascontiguousarray(tris, np.int32)
    cid = np.ascontiguousarray(cid, np.int32)
    cpos = np.ascontiguousarray(cpos, np.float64).reshape(-1, 3)
    prm = _abi.ArapDeformParams()
    prm.max_iter, prm.energy, prm.smoothed_alpha = max_iter, energy, 0.01
    rep = _abi.ArapDeformReport()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = ctx.lib.deftri_arap_deform(ctx.h, len(v), dp(v), len(tris), ip(tris), len(cid), ip(cid), len(cpos), dp(cpos),
                                    C.byref(prm), dp(out), None, C.byref(rep))
    return rc, rep


def test_a_component_without_a_constraint_is_refused_before_any_solve(host):
    a = np.array([[0.0, 0.0, 2.0], [1.0, 0.1, 2.1], [0.3, 0.9, 1.9]])
    v = np.r_[a, a + [3.0, 0.0, 0.0]]
    tris = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    out = np.full((6, 3), -7.0)
    rc, rep = _raw_call(host, v, tris, [0], v[:1] + 0.5, out=out)
    assert rc == E_GRAPH
    assert b"component" in host.lib.deftri_last_error(host.h)
    assert np.all(out == -7.0)
    assert rep.iterations == 0 and rep.cg_iterations == 0           # returned at once
    # a constraint in each triangle: solvable
    rc, rep = _raw_call(host, v, tris, [0, 3], np.r_[v[:1] + 0.5, v[3:4] - 0.5], out=out)
    assert rc == 0 and rep.n_constraints == 2


def test_argument_errors_leave_the_output_untouched(host):
    v, tris = cases.mesh(65)
    ids, pos = ref.four_handles(v)
    out = np.full((65, 3), -7.0)
    bad_tris = tris.copy()
    bad_tris[3, 1] = 65
    for args, kw in (((v, tris, np.zeros(0, np.int32), pos), {}),                   # no constraints
                     ((v, tris, ids, np.zeros((0, 3))), {}),                         # no constraint positions
                     ((v, tris, np.r_[ids[:3], [65]], pos), {}),                     # a constraint index out of range
                     ((v, tris, np.r_[ids[:3], [-1]], pos), {}),
                     ((v, bad_tris, ids, pos), {}),                                  # a triangle index out of range
                     ((v, tris, ids, pos), {"energy": 2}),                           # a bad energy
                     ((v, tris, ids, pos), {"max_iter": -1}),
                     ((v[:2], tris[:0], [0], pos[:1]), {})):                         # n < 3
        o = out[:len(args[0])]
        rc, _ = _raw_call(host, *args, out=o, **kw)
        assert rc == E_ARG, (rc, kw)
        assert host.lib.deftri_last_error(host.h)
        assert np.all(out == -7.0)


def test_a_global_step_that_does_not_converge_is_an_error(host):
    v, tris = cases.mesh(65)
    ids, pos = ref.four_handles(v)
    with pytest.raises(capi.DeftriError) as e:
        host.arap_deform(v, tris, ids, pos, max_iter=20, cg_max_iterations=1)
    assert e.value.code == E_NUMERIC
    assert e.value.report["cg_unconverged_steps"] >= 1


def test_map_entry_moves_keyframe_2_as_the_reference_does(host):
    cases.check_map_entry(host)


def test_map_entry_refuses_a_slot_the_reference_would_dereference(host):
    m = cases.two_view_map()
    order = m.kf_order()
    kf2 = m.keyframes[order[0]]
    kf2.map_points[7] = None                 # v2MPs[7] is null where invertedPosIndexes1 holds 7
    before = copy.deepcopy(m)
    with pytest.raises(capi.DeftriError) as e:
        host.arap_open3d_optimization(m)
    assert e.value.code == E_ARG
    for kid in order:
        assert np.array_equal(cases.positions(m, kid), cases.positions(before, kid))


def _settings(n_optimizations):
    s = Settings()
    s.selection = "open3DArap"
    s.n_optimizations = n_optimizations
    if s.depth_weight == 0.0:
        s.depth_weight = 3.0
    return s


@pytest.mark.parametrize("native", [True, False])
def test_deformation_optimization_runs_every_round(host, native, monkeypatch):
    monkeypatch.setattr(optimization, "_ctx", lambda device=0: host)
    m = cases.two_view_map()
    direct = copy.deepcopy(m)
    log = []
    rounds = optimization.deformationOptimization(m, _settings(2), native=native, log=log.append)
    assert rounds == [{"round": 1, "update": 100.0}, {"round": 2, "update": 100.0}] and log == rounds
    host.arap_open3d_optimization(direct)
    host.arap_open3d_optimization(direct)
    for kid in m.kf_order():
        assert np.array_equal(cases.positions(m, kid), cases.positions(direct, kid))
    once = cases.two_view_map()
    host.arap_open3d_optimization(once)
    assert not np.array_equal(cases.positions(once, m.kf_order()[0]), cases.positions(m, m.kf_order()[0]))


def test_abi_sizes():
    lib = capi.load()
    assert lib.deftri_abi_version() == 8
    assert lib.deftri_sizeof(25) == C.sizeof(_abi.ArapDeformParams) == 32
    assert lib.deftri_sizeof(26) == C.sizeof(_abi.ArapDeformReport) == 88
    for name in ("deftri_arap_deform", "deftri_arap_open3d_optimization"):
        assert name in capi.EXPORTED
