"""deftri_arap_deform and deftri_arap_open3d_optimization on a device context (csrc/arap_deform.hip): the
cases and bounds of tests/test_arap_deform.py, more than one block of partials, bit-identical repeats, and the device
against the host-only context."""
import numpy as np
import pytest

import arap_deform_cases as cases
from deftri import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    with capi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def host():
    with capi.Context(-1) as c:
        yield c


@pytest.mark.parametrize("energy", ["spokes", "smoothed"])
@pytest.mark.parametrize("n", [65, 257])
def test_four_handles_against_the_lu_reference(dev, host, n, energy):
    p, en, rep = cases.check_four_handles(dev, n, energy)
    assert rep["on_device"] == 1
    # the device against the host-only context: within the same bound
    ids, pos, p_ref, _, cond = cases.four_handle_reference(n, energy, 20)
    v, tris = cases.mesh(n)
    ph, enh, reph = host.arap_deform(v, tris, ids, pos, max_iter=20, energy=energy)
    assert reph["on_device"] == 0
    assert np.abs(p - ph).max() <= cases.position_bound(cond, p_ref)
    assert np.abs(en / enh - 1.0).max() <= 1e-8
    assert rep["area"] == pytest.approx(reph["area"], rel=1e-14)


@pytest.mark.parametrize("energy", ["spokes", "smoothed"])
def test_several_blocks_of_partials(dev, energy):
    """n = 1025: five 256-thread blocks, the last with one vertex."""
    _, _, rep = cases.check_four_handles(dev, 1025, energy, iters=5)
    assert rep["on_device"] == 1


@pytest.mark.parametrize("n", [65, 257])
def test_the_references_own_arguments_translate_the_mesh(dev, n):
    cases.check_reference_arguments(dev, n)


def test_three_vertices_three_constraints(dev):
    v, tris = cases.mesh(3)
    cpos = v[::-1] + 0.25
    p, _, rep = dev.arap_deform(v, tris, [0, 1, 2], cpos, max_iter=5)
    assert np.array_equal(p, cpos)
    assert rep["n_free"] == 0 and rep["cg_iterations"] == 0 and rep["on_device"] == 1


@pytest.mark.parametrize("energy", ["spokes", "smoothed"])
def test_two_calls_are_bit_identical_whatever_the_flag_batch(dev, energy, monkeypatch):
    ids, pos, _, _, _ = cases.four_handle_reference(257, energy, 20)
    v, tris = cases.mesh(257)
    p1, e1, r1 = dev.arap_deform(v, tris, ids, pos, max_iter=20, energy=energy)
    p2, e2, r2 = dev.arap_deform(v, tris, ids, pos, max_iter=20, energy=energy)
    assert np.array_equal(p1, p2) and np.array_equal(e1, e2)
    assert r1["cg_iterations"] == r2["cg_iterations"]
    # the host reads the flags every 7 iterations instead of every 32: the same bits and counts
    monkeypatch.setenv("DEFTRI_ARAP_CG_BATCH", "7")
    p3, e3, r3 = dev.arap_deform(v, tris, ids, pos, max_iter=20, energy=energy)
    assert np.array_equal(p1, p3) and np.array_equal(e1, e3)
    assert r1["cg_iterations"] == r3["cg_iterations"] and r1["cg_max_in_step"] == r3["cg_max_in_step"]


def test_a_global_step_that_does_not_converge_is_an_error(dev):
    ids, pos, _, _, _ = cases.four_handle_reference(65, "spokes", 20)
    v, tris = cases.mesh(65)
    with pytest.raises(capi.DeftriError) as e:
        dev.arap_deform(v, tris, ids, pos, max_iter=20, cg_max_iterations=1)
    assert e.value.code == -4 and e.value.report["cg_unconverged_steps"] >= 1


def test_map_entry_moves_keyframe_2_as_the_reference_does(dev):
    m, rep = cases.check_map_entry(dev)
    assert rep["on_device"] == 1
    # the mesh builder switch at 1 (stars on the device): the same map
    try:
        m1, _ = cases.check_map_entry(dev, prepare=lambda c: c.set_mesh_builder(1))
    finally:
        dev.set_mesh_builder(0)
    for kid in m.kf_order():
        assert np.array_equal(cases.positions(m, kid), cases.positions(m1, kid))
