"""deftri_set_tile_builder(1) on the device (csrc/plan_dev.hip): the one-pair tile layout — groups and edges
by group, the partition, entries and slots, cross slots — built by kernels, against build_tiles of csrc/spcg_tile.cpp
array by array (all 33 digests of deftri_debug_plan_digest), then through an upload with an LM solve and through the
drop-in arapOptimization call, bit for bit.

Sizes: the sizes of the plan builder's test (the scans' 2048-element tiles, the radix sort's 256 groups).  Up to 65
correspondences the layout is one tile without cut edges; from 255 on (checked on a host-only context below: 257 is
not the first such size) there are several tiles, halo rows and cross slots."""
import copy
import dataclasses

import numpy as np
import pytest

from deftri import capi, sim

pytestmark = pytest.mark.gpu

W = (1.0, 2e5, np.float32(0.003))
FNV_BASIS = 1469598103934665603          # the digest of an empty array
ALL_STAGES, ROW_STAGES = 0b1111111111, 0b000111


@pytest.fixture(scope="module")
def ctxs():
    with capi.Context(-1) as h, capi.Context(0) as d:
        yield h, d


@pytest.fixture(scope="module")
def cloud():
    """A compacted two-view scene: a prefix of it is a scene of exactly that many correspondences."""
    _, gt = sim.simulate_two_view(n=3200, seed=11, compact=True)
    assert len(gt["original"]) >= 2049
    return gt["original"], gt["moved"]


def graph_of(host, cloud, n):
    """the graph of exactly n correspondences (n groups, 2 n points); above the cloud's size: of about n"""
    orig, moved = cloud
    if n > len(orig):
        m, _ = sim.simulate_two_view(n=n, seed=12, compact=True)
        return host.build_graph(m, *W)
    m, gt = sim.simulate_two_view(orig=orig[:n], moved=moved[:n], compact=True)
    assert len(gt["original"]) == n and gt["valid"].all()
    p = host.build_graph(m, *W)
    assert p.n_points == 2 * n and p.n_pairs == 1
    return p


def compare(dev, p, tile=1, plan_builder=1):
    """(plan builder 1, tile builder 1) against mode 0 on one device context, all 33 digests; returns the build's info
    and the digests by name"""
    dev.set_tile_builder(0)
    names, want = dev.debug_plan_digest(p, 0, tile)
    info0 = dev.plan_build_info()
    assert (info0["builder_used"], info0["stages"], info0["reason"]) == (0, 0, 0)
    dev.set_tile_builder(1)
    try:
        _, got = dev.debug_plan_digest(p, plan_builder, tile)
        info = dev.plan_build_info()
    finally:
        dev.set_tile_builder(0)
    assert len(got) == 33
    for name, a, b in zip(names, want, got):
        assert a == b, f"{name} differs ({info})"
    return info, dict(zip(names, got))


def assert_built(info, stages=ALL_STAGES):
    assert (info["builder_used"], info["reason"], info["stages"]) == (1, 0, stages), info


def assert_refused(info, digests):
    """build_tiles refused the layout: the device tile stages stopped, the host went on from the device's rows"""
    assert digests["tile_tab"] == FNV_BASIS
    assert_built(info, ROW_STAGES)


@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 2047, 2048, 2049])
def test_two_view_graphs(ctxs, cloud, n):
    host, dev = ctxs
    p = graph_of(host, cloud, n)
    if n >= 257:
        names, want = host.debug_plan_digest(p, 0, 1)
        assert dict(zip(names, want))["tile_xdst"] != FNV_BASIS      # several tiles, cut edges
    info, digests = compare(dev, p)
    assert_built(info)
    assert (digests["tile_xdst"] != FNV_BASIS) == (n >= 255)


def test_5000_twice_on_one_context(ctxs, cloud):
    """the same graph before and after a smaller build: the arenas are reused, the result does not change"""
    host, dev = ctxs
    p, small = graph_of(host, cloud, 5000), graph_of(host, cloud, 64)
    first, d1 = compare(dev, p)
    assert_built(first)
    assert d1["tile_xdst"] != FNV_BASIS
    assert_built(compare(dev, small)[0])
    second, d2 = compare(dev, p)
    assert_built(second)
    assert d1 == d2


@pytest.fixture(scope="module")
def p300(ctxs, cloud):
    return graph_of(ctxs[0], cloud, 300)


def edited(p, **kw):
    q = dataclasses.replace(p, **kw)
    assert q.validate()
    return q


def relink(ap, links):
    """every link (a, b) becomes the union pair (columns 0, 1) of an edge of its own that holds neither point yet"""
    e = 0
    for a, b in links:
        while a in ap[e, 2:] or b in ap[e, 2:]:
            e += 1
        ap[e, 0], ap[e, 1] = a, b
        e += 3


def test_unit_cap(ctxs, p300):
    """300 more points that no edge touches: groups of one row without edges, spread over the mesh plane, so tiles
    close on the 128 units of a tile long before its LDS estimate is reached"""
    rng = np.random.default_rng(5)
    lo, hi = p300.order_xy.min(0), p300.order_xy.max(0)
    xy = lo + (hi - lo) * rng.random((300, 2))
    q = edited(p300, points=np.vstack([p300.points, np.column_stack([xy, np.full(300, 0.3)])]),
               order_xy=np.vstack([p300.order_xy, xy]))
    assert q.n_points == p300.n_points + 300
    info, digests = compare(ctxs[1], q)
    assert_built(info)
    assert digests["tile_xdst"] != FNV_BASIS


def test_all_keys_tie(ctxs, p300):
    assert_built(compare(ctxs[1], edited(p300, order_xy=np.full_like(p300.order_xy, 0.25)))[0])


def test_nan_and_inf_coordinates(ctxs, p300):
    xy = p300.order_xy.copy()
    a = p300.arap_pts[0]
    xy[min(a[0], a[1]), 0] = np.nan                  # the representatives (smallest ids) of edge 0's two groups
    xy[min(a[2], a[3]), 1] = np.inf
    xy[p300.n_points - 1] = (-np.inf, np.nan)
    assert_built(compare(ctxs[1], edited(p300, order_xy=xy))[0])


def test_without_order_xy(ctxs, p300):
    assert_built(compare(ctxs[1], edited(p300, order_xy=None))[0])


def test_refused_groups_of_more_than_two_rows(ctxs, p300):
    """the chain (a group of 10) and the group of 70 points of the plan builder's test"""
    ap = p300.arap_pts.copy()
    firsts = np.unique(ap[:, 0])                      # one copy of every vertex
    chain = firsts[-5:][::-1]
    big = firsts[:70:2][:35]
    relink(ap, [(chain[k], chain[k + 1]) for k in range(4)] + [(big[k + 1], big[0]) for k in range(34)])
    assert_refused(*compare(ctxs[1], edited(p300, arap_pts=ap)))


def test_refused_vertex_with_65_out_edges(ctxs, p300):
    """the i columns of other vertices' edges rewritten to vertex 0's copies until it has 65 out-edges (the problem's
    validate() admits it)"""
    ap = p300.arap_pts.copy()
    v = ap[0, :2].copy()
    have = int((ap[:, 0] == v[0]).sum())
    others = [e for e in range(len(ap)) if ap[e, 0] != v[0] and not set(ap[e, 2:]) & set(v)]
    for e in others[:65 - have]:
        ap[e, :2] = v
    assert (ap[:, 0] == v[0]).sum() == 65
    assert_refused(*compare(ctxs[1], edited(p300, arap_pts=ap)))


def test_duplicated_edge(ctxs, p300):
    """an ARAP edge listed twice (validate() admits it) is no refusal: edge 0 appended once more, and every edge of
    the graph doubled, the cut edges among them (two edges of one vertex into the same halo group)"""
    for rep in (np.r_[np.arange(len(p300.arap_pts)), 0], np.repeat(np.arange(len(p300.arap_pts)), 2)):
        q = edited(p300, arap_pts=p300.arap_pts[rep], arap_pair=p300.arap_pair[rep], arap_rot=p300.arap_rot[rep],
                   arap_w=p300.arap_w[rep])
        info, digests = compare(ctxs[1], q)
        assert_built(info)
        assert digests["tile_xdst"] != FNV_BASIS


def test_run_above_the_bound_builds_on_the_host(ctxs, p300):
    """a group of 260 points: the row sort's bound, so the whole plan is the host's"""
    ap = p300.arap_pts.copy()
    firsts = np.unique(ap[:, 0])
    relink(ap, [(firsts[k + 1], firsts[0]) for k in range(129)])
    info, _ = compare(ctxs[1], edited(p300, arap_pts=ap))
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 2), info


def test_not_applicable_eight_keyframes(ctxs):
    host, dev = ctxs
    p = host.build_graph(sim.multi_view_arrays(n=120, k=8), *W)
    assert p.n_pairs == 28
    info, _ = compare(dev, p)
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 1)


def test_not_applicable_without_the_tile_layout(ctxs, p300):
    info, _ = compare(ctxs[1], p300, tile=0)
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 1)


def test_no_effect_with_plan_builder_0(ctxs, p300):
    info, _ = compare(ctxs[1], p300, plan_builder=0)
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 0)


@pytest.fixture(scope="module")
def scene20k():
    m, _ = sim.simulate_two_view(n=20000, seed=4, scale_scene=True, compact=True)
    return m


def test_upload_and_lm_solve_bit_for_bit(ctxs, scene20k):
    p = ctxs[0].build_graph(scene20k, *W)
    assert p.n_unknowns >= 100000
    out = []
    for mode in (0, 1):
        with capi.Context(0) as c:
            c.set_plan_builder(mode)
            c.set_tile_builder(mode)
            c.set_linear_solver("pcg")
            c.upload(p)
            r = c.solve_lm(5)
            out.append((r, c.download(), c.plan_info(), c.plan_build_info()))
    (r0, s0, i0, b0), (r1, s1, i1, b1) = out
    assert i0["plan"] == i1["plan"] and i0 == i1
    assert b0["builder_used"] == 0 and b0["reason"] == 0
    assert_built(b1)
    for k in ("chi2_iter", "trials_iter", "lambda_final", "chi2_initial", "chi2_final", "iterations", "pcg_iterations"):
        assert np.array_equal(np.asarray(r0[k]), np.asarray(r1[k])), k
    for a, b, what in zip(s0, s1, ("points", "scales", "T_g")):
        assert np.array_equal(a, b), what


def map_state(m):
    pos = np.array([mp.position for mp in m.map_points.values()])
    scales = np.array([kf.estimated_depth_scale for kf in m.keyframes.values()])
    tg = np.array([m.global_T[k].as7() for k in sorted(m.global_T)])
    return pos, scales, tg


def test_through_arap_optimization_twice(scene20k):
    """the second call is the next round: the written-back points have moved, so mesh, graph and plan are rebuilt"""
    ma, mb = copy.deepcopy(scene20k), copy.deepcopy(scene20k)
    with capi.Context(0) as a, capi.Context(0) as b:
        b.set_mesh_builder(1)
        b.set_plan_builder(1)
        b.set_tile_builder(1)
        before = map_state(ma)[0]
        for call in range(2):
            a.arap_optimization(ma, 1.0, 50.0, 2e5, 0.0, 0.0, np.float32(0.003), 3)
            b.arap_optimization(mb, 1.0, 50.0, 2e5, 0.0, 0.0, np.float32(0.003), 3)
            sa, sb = map_state(ma), map_state(mb)
            for x, y, what in zip(sa, sb, ("positions", "depth scales", "T_g")):
                assert np.array_equal(x, y), (call, what)
            assert not np.array_equal(sa[0], before)
            before = sa[0]
            assert_built(b.plan_build_info())
            assert a.plan_build_info()["builder_used"] == 0
