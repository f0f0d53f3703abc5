"""deftri_delaunay2d on the device (csrc/delaunay_dev.hip: one wave per star, the predicates' floating-point filters,
marked stars rebuilt on the host) against the host-only context's exact stars and the host sweep: the triangles,
hull_size, skipped and fallback are equal on every input; on clean inputs the device builds every star itself."""
import copy

import numpy as np
import pytest

import delaunay_ref as ref
from deftri import capi, sim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs():
    with capi.Context(-1) as h, capi.Context(0) as d:
        yield h, d


def both(ctxs, xy):
    h, d = ctxs
    (th, rh), (td, rd) = h.delaunay(xy), d.delaunay(xy)
    assert np.array_equal(th, td)
    for k in ("n_tris", "hull_size", "skipped", "fallback"):
        assert rh[k] == rd[k], (k, rh, rd)
    return td, rd


@pytest.mark.parametrize("name", sorted(ref.CLEAN))
def test_device_equals_host(ctxs, name):
    xy = ref.CLEAN[name]()
    tris, rep = both(ctxs, xy)
    want, hull, _ = ref.sweep(xy)
    assert np.array_equal(tris, want) and rep["hull_size"] == hull
    assert rep["path"] == 2 and rep["fallback"] == 0 and rep["round_trips"] == 1
    if name in ref.RANDOM_CLOUDS:
        # no predicate of a random cloud is within its filter's bound: the device builds every star itself (a
        # device path that always fell back would pass the equality above)
        assert rep["host_stars"] == 0, rep
    if name == "circle_with_centre":
        # the centre's star has 100 neighbours, above the 64 the device holds: marked, rebuilt on the host, merged
        assert rep["host_stars"] >= 1 and rep["max_degree"] == 100
    if name == "gaussian2000":
        assert ref.still_valid(xy, tris) == 1


# 1023 .. 2500: the chunk boundaries of the rows' scan, one workgroup of 1024 threads (3 is its one-thread case)
@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 129, 1023, 1024, 1025, 2500])
def test_wave_and_tournament_boundaries(ctxs, n):
    xy = ref.gaussian(n, 20 + n)
    tris, rep = both(ctxs, xy)
    assert np.array_equal(tris, ref.sweep(xy)[0])
    assert rep["path"] == 2 and rep["host_stars"] == 0 and rep["fallback"] == 0


def test_one_crowded_cell(ctxs):
    xy = ref.crowded_cell()
    tris, rep = both(ctxs, xy)
    assert np.array_equal(tris, ref.sweep(xy)[0]) and rep["path"] == 2 and rep["fallback"] == 0


def test_near_tie_marks_four_stars_and_merges_them(ctxs):
    """(0,0), (1,0), (1,1), (0, 1 + 2^-50): the in-circle filter cannot decide the square's diagonal in the four
    stars that meet it, and no predicate is exactly zero: the host rebuilds those stars and their rows are merged."""
    xy = ref.near_tie()
    tris, rep = both(ctxs, xy)
    assert np.array_equal(tris, ref.sweep(xy)[0])
    assert rep["host_stars"] >= 4 and rep["fallback"] == 0 and rep["path"] == 2


def test_fallbacks_equal_the_host(ctxs):
    _, rep = both(ctxs, ref.exact_lattice(8))
    assert rep["fallback"] == 1
    _, rep = both(ctxs, ref.with_duplicate())
    assert rep["fallback"] == 2 and rep["skipped"] == 1
    _, rep = both(ctxs, np.array([[0.0, 0.0], [1.0, 2.0]]))
    assert rep["fallback"] == 4
    for c in ctxs:
        with pytest.raises(capi.DeftriError) as e:
            c.delaunay(ref.line())
        assert e.value.code == -6


FIELDS = ("points", "tg", "scales", "cam_kb8", "cam_pose", "rep_point", "rep_cam", "rep_obs", "rep_info",
          "dep_point", "dep_scale", "dep_cam", "dep_meas", "dep_info", "arap_pts", "arap_pair", "arap_rot",
          "arap_w", "rot", "pair_area", "pair_info", "order_xy", "point_ids")


def same(pa, pb, skip=()):
    for f in FIELDS:
        if f not in skip:
            assert np.array_equal(getattr(pa, f), getattr(pb, f)), f


@pytest.mark.parametrize("scene", ["two_view", "three_keyframes"])
def test_mesh_builder_1_against_0(scene):
    m = sim.simulate_two_view(n=300, seed=3)[0] if scene == "two_view" else sim.simulate_multi_view(n=200, k=3, seed=4)[0]
    w = (1.0, 2e5, np.float32(0.003))
    with capi.Context(0) as a, capi.Context(0) as b:
        b.set_mesh_builder(1)
        p0 = a.build_graph(m, *w)
        same(p0, b.build_graph(copy.deepcopy(m), *w))
        # arapOptimization writes the same map, bit for bit
        ma, mb = copy.deepcopy(m), copy.deepcopy(m)
        a.arap_optimization(ma, 1.0, 50.0, 2e5, 0.0, 0.0, np.float32(0.003), 1)
        b.arap_optimization(mb, 1.0, 50.0, 2e5, 0.0, 0.0, np.float32(0.003), 1)
        pa, pb = a.build_graph(ma, *w), b.build_graph(mb, *w)
        same(pa, pb)
        assert not np.array_equal(pa.points, p0.points)
        # the memos come first, as before: the same map again is answered by the graph memo
        assert a.graph_stats()[:2] == b.graph_stats()[:2]
        hits = b.graph_stats()[0]
        same(pb, b.build_graph(mb, *w))
        assert b.graph_stats()[0] == hits + 1
        assert a.graph_repairs() == b.graph_repairs() == (0, 0)


def test_mesh_builder_1_second_call_with_moved_points():
    """A second build with moved points: the structure memo (a tiny motion) and a new triangulation (a large one)
    both equal the host sweep's graph."""
    n = 200
    m = sim.multi_view_arrays(n=n, k=3, seed=4)
    rng = np.random.default_rng(5)
    with capi.Context(0) as a, capi.Context(0) as b:
        b.set_mesh_builder(1)
        p0 = a.build_graph(m, 1.0, 2e5, np.float32(0.003))
        same(p0, b.build_graph(m, 1.0, 2e5, np.float32(0.003)))
        ext = np.abs(p0.points).max()
        for scale in (1e-9, 3e-2):
            m2 = copy.deepcopy(m)
            pts = p0.points + rng.normal(0.0, scale * ext, p0.points.shape)
            for pid, x in zip(p0.point_ids, pts):
                m2.kfs[int(pid) // n]["pos"][int(pid) % n] = np.asarray(x, np.float32)
            sa, sb = a.graph_stats()[1], b.graph_stats()[1]
            pa, pb = a.build_graph(m2, 1.5, 1e5, np.float32(0.004)), b.build_graph(m2, 1.5, 1e5, np.float32(0.004))
            same(pa, pb)
            assert (a.graph_stats()[1] > sa) == (b.graph_stats()[1] > sb)
            m, p0 = m2, pa
