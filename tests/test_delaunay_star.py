"""deftri_delaunay2d on a host-only context: every star built by csrc/delaunay_star.h with the exact predicates, in a
sequential loop.  Checked against the definition in exact rational arithmetic (tests/delaunay_ref.py)
and, triangle for triangle, against the library's host sweep (delaunay2d), with the fallbacks of ties, duplicates,
collinear input and too few points, and the C-ABI's sizes and refusals."""
import copy
import ctypes as C

import numpy as np
import pytest

import delaunay_ref as ref
from deftri import _abi, capi, sim


@pytest.fixture(scope="module")
def host():
    with capi.Context(-1) as c:
        yield c


def check_against_sweep(ctx, xy, fallback=0):
    tris, rep = ctx.delaunay(xy)
    want, hull, skipped = ref.sweep(xy)
    assert np.array_equal(tris, want)
    assert (rep["n_tris"], rep["hull_size"], rep["skipped"], rep["fallback"]) == (len(want), hull, skipped, fallback), rep
    return tris, rep


@pytest.mark.parametrize("name", ["three", "quadrilateral", "inside", "gaussian30"])
def test_against_the_definition(host, name):
    xy = {"three": np.array([[0.0, 0.0], [1.0, 0.1], [0.3, 0.9]]),
          "quadrilateral": np.array([[0.0, 0.0], [2.0, 0.1], [2.3, 1.4], [-0.2, 1.1]]),
          "inside": np.array([[0.0, 0.0], [4.0, 0.0], [1.0, 3.0], [1.5, 1.0]]),
          "gaussian30": ref.gaussian(30, 9)}[name]
    want = ref.oracle(xy)
    assert not isinstance(want, str)
    tris, rep = host.delaunay(xy)
    assert np.array_equal(tris, want)
    assert rep["path"] == 1 and rep["fallback"] == 0 and rep["n_tris"] == len(want)
    assert rep["hull_size"] == 2 * len(xy) - 2 - len(want)          # Euler: T = 2 n - 2 - h


def test_the_oracle_sees_ties():
    assert ref.oracle(ref.exact_lattice(3)) == "ties"


@pytest.mark.parametrize("name", sorted(ref.CLEAN))
def test_equals_the_sweep(host, name):
    xy = ref.CLEAN[name]()
    tris, rep = check_against_sweep(host, xy)
    assert rep["path"] == 1 and rep["host_stars"] == len(xy) and rep["round_trips"] == 0
    assert ref.still_valid(xy, tris) == 1
    if name == "circle_with_centre":
        assert rep["max_degree"] == 100
    if name == "jittered_lattice":
        assert len(xy) == 400


@pytest.mark.parametrize("name", ["crowded_cell", "near_tie"])
def test_equals_the_sweep_on_the_device_tests_inputs(host, name):
    check_against_sweep(host, getattr(ref, name)())


def test_exact_lattice_falls_back_on_a_tie(host):
    _, rep = check_against_sweep(host, ref.exact_lattice(8), fallback=1)
    assert rep["path"] == 0


def test_duplicate_falls_back(host):
    xy = ref.with_duplicate()
    _, rep = check_against_sweep(host, xy, fallback=2)
    assert rep["path"] == 0 and rep["skipped"] == ref.sweep(xy)[2] == 1


def test_collinear_is_a_graph_error(host):
    assert ref.sweep(ref.line()) is None
    with pytest.raises(capi.DeftriError) as e:
        host.delaunay(ref.line())
    assert e.value.code == _abi.DEFTRI_E_GRAPH


def test_two_points(host):
    tris, rep = host.delaunay(np.array([[0.0, 0.0], [1.0, 2.0]]))
    assert len(tris) == 0 and rep["fallback"] == 4 and rep["path"] == 0 and rep["n_tris"] == 0


def test_abi_and_refusals(host):
    lib = capi.load()
    assert lib.deftri_sizeof(24) == C.sizeof(_abi.DelaunayReport) == 64
    assert lib.deftri_abi_version() == 8
    for name in ("deftri_delaunay2d", "deftri_set_mesh_builder"):
        assert name in capi.EXPORTED and hasattr(lib, name)
    xy = ref.gaussian(65, 1)
    need = len(ref.sweep(xy)[0])
    tris = np.full((need, 3), -7, np.int32)
    rep = _abi.DelaunayReport()
    rep.n_tris = -7
    dp, ip = xy.ctypes.data_as(C.POINTER(C.c_double)), tris.ctypes.data_as(C.POINTER(C.c_int32))
    rc = lib.deftri_delaunay2d(host.h, len(xy), dp, need - 1, ip, C.byref(rep))
    assert rc == _abi.DEFTRI_E_ARG and str(need).encode() in lib.deftri_last_error(host.h)
    assert (tris == -7).all() and rep.n_tris == -7
    assert lib.deftri_delaunay2d(host.h, len(xy), dp, need, ip, C.byref(rep)) == 0 and rep.n_tris == need
    assert lib.deftri_delaunay2d(host.h, len(xy), None, need, ip, C.byref(rep)) == _abi.DEFTRI_E_ARG
    assert lib.deftri_delaunay2d(host.h, len(xy), dp, need, None, C.byref(rep)) == _abi.DEFTRI_E_ARG
    assert lib.deftri_delaunay2d(host.h, len(xy), dp, need, ip, None) == _abi.DEFTRI_E_ARG
    bad = xy.copy()
    bad[11, 1] = np.inf
    before = tris.copy()
    rc = lib.deftri_delaunay2d(host.h, len(bad), bad.ctypes.data_as(C.POINTER(C.c_double)), need, ip, C.byref(rep))
    assert rc == _abi.DEFTRI_E_ARG and b"finite" in lib.deftri_last_error(host.h) and np.array_equal(tris, before)
    with pytest.raises(capi.DeftriError):
        host.set_mesh_builder(2)


FIELDS = ("points", "tg", "scales", "cam_kb8", "cam_pose", "rep_point", "rep_cam", "rep_obs", "rep_info",
          "dep_point", "dep_scale", "dep_cam", "dep_meas", "dep_info", "arap_pts", "arap_pair", "arap_rot",
          "arap_w", "rot", "pair_area", "pair_info", "order_xy", "point_ids")


@pytest.mark.parametrize("scene", ["two_view", "three_keyframes"])
def test_mesh_builder_on_the_host_builds_the_same_graph(scene):
    m = sim.simulate_two_view(n=300, seed=3)[0] if scene == "two_view" else sim.multi_view_arrays(n=200, k=3, seed=4)
    with capi.Context(-1) as a, capi.Context(-1) as b:
        b.set_mesh_builder(1)
        pa, pb = a.build_graph(m, 1.0, 2e5, np.float32(0.003)), b.build_graph(copy.deepcopy(m), 1.0, 2e5, np.float32(0.003))
        for f in FIELDS:
            assert np.array_equal(getattr(pa, f), getattr(pb, f)), f
        assert a.graph_stats()[:2] == b.graph_stats()[:2] == (0, 0) and b.graph_repairs() == (0, 0)
