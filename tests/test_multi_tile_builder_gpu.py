"""deftri_set_multi_tile_builder(1) on the device (csrc/plan_dev.hip): the tile layout of several keyframe
pairs — the (pair, group) units in each pair's own Morton order, the edges by unit, the partition per pair, entries,
slots, own rows, shares and cross slots — built by kernels, against build_tiles_multi of csrc/spcg_tile.cpp array by
array: all 33 digests of deftri_debug_plan_digest and the 6 of deftri_debug_plan_tile_digest (tile_trow, tile_tdst,
tile_poff, tile_nshare and the tile scalars, which the 33 leave out), then through an upload with an LM solve and
through the drop-in arapOptimization call, bit for bit.

Sizes: P = n k points.  One tile per pair up to n = 85 (P = 255 and 256 around the radix sort's workgroup), cut edges
from n = 129 (6 tiles), 12 tiles at (200, 4), 84 tiles of 28 pairs at (300, 8) where a row lies in 7 pairs (6 share
planes), P = 2049 around the scan's tile at (683, 3)."""
import copy
import dataclasses

import numpy as np
import pytest

from deftri import _abi, capi, sim

pytestmark = pytest.mark.gpu

W = (1.0, 1e7, np.float32(0.3))
FNV_BASIS = 1469598103934665603          # the digest of an empty array
TILE_STAGES, LAYOUT_STAGES, ROW_STAGES = 0x3ff, 0x1bff, 0b111
SWITCHES = ("set_plan_builder", "set_tile_builder", "set_layout_builder", "set_multi_pair_builder", "set_multi_tile_builder")
EDGE_ARRAYS = ("arap_pts", "arap_pair", "arap_rot", "arap_w")


@pytest.fixture(scope="module")
def ctxs():
    with capi.Context(-1) as h, capi.Context(0) as d:
        yield h, d


_graphs = {}


def graph_of(host, n, k):
    """the all-pairs graph of n correspondences in k keyframes, built once per module"""
    if (n, k) not in _graphs:
        p = host.build_graph(sim.multi_view_arrays(n=n, k=k), *W)
        assert p.n_points == n * k and p.n_pairs == k * (k - 1) // 2 and p.n_scales == 2 * p.n_pairs
        _graphs[n, k] = p
    return _graphs[n, k]


def compare(dev, p, tile=1, plan_builder=1, multi=1, multi_tile=1, layout=0, tile_builder=0):
    """mode 0 against plan builder 1 with the multi-pair and multi-tile builders (and the others as given) on one
    device context: all 33 digests and the 6 tile digests; returns the build's info and the digests by name.  The
    switches are put back"""
    for f in SWITCHES:
        getattr(dev, f)(0)
    names, want = dev.debug_plan_digest(p, 0, tile)
    tnames, twant = dev.debug_plan_tile_digest(p, 0, tile)
    info0 = dev.plan_build_info()
    assert (info0["builder_used"], info0["stages"], info0["reason"]) == (0, 0, 0)
    dev.set_multi_pair_builder(multi)
    dev.set_multi_tile_builder(multi_tile)
    dev.set_layout_builder(layout)
    dev.set_tile_builder(tile_builder)
    try:
        _, got = dev.debug_plan_digest(p, plan_builder, tile)
        info = dev.plan_build_info()
        _, tgot = dev.debug_plan_tile_digest(p, plan_builder, tile)
        tinfo = dev.plan_build_info()
    finally:
        for f in SWITCHES:
            getattr(dev, f)(0)
    assert len(got) == 33 and len(tgot) == 6
    for name, a, b in zip(names + tnames, want + twant, got + tgot):
        assert a == b, f"{name} differs ({info})"
    assert triple(info) == triple(tinfo), (info, tinfo)
    return info, dict(zip(names + tnames, got + tgot))


def triple(info):
    return info["builder_used"], info["reason"], info["stages"]


def assert_built(info, digests, stages=TILE_STAGES):
    assert digests["tile_tab"] != FNV_BASIS and digests["tile_trow"] != FNV_BASIS      # the host accepts the graph
    assert triple(info) == (1, 0, stages), info


def assert_refused(info, digests):
    """build_tiles_multi refuses the graph: the device's rows, the host's rest"""
    assert digests["tile_tab"] == FNV_BASIS and digests["tile_trow"] == FNV_BASIS
    assert triple(info) == (1, 0, ROW_STAGES), info


@pytest.mark.parametrize("n,k", [(3, 3), (4, 3), (9, 3), (64, 4), (85, 3), (129, 3), (200, 4), (300, 8), (683, 3), (1025, 3)])
def test_all_pairs_graphs(ctxs, n, k):
    host, dev = ctxs
    info, digests = compare(dev, graph_of(host, n, k))
    assert_built(info, digests)
    for name in ("tile_tdst", "tile_poff", "tile_nshare"):
        assert digests[name] != FNV_BASIS, name
    if n >= 129:
        assert digests["tile_xdst"] != FNV_BASIS and digests["tile_halo"] != FNV_BASIS


def test_windowed_graph(ctxs):
    host, dev = ctxs
    host.set_pair_window(2)
    try:
        p = host.build_graph(sim.multi_view_arrays(n=120, k=20), *W)
    finally:
        host.set_pair_window(0)
    assert p.n_pairs == 37 and p.n_scales == 74
    assert_built(*compare(dev, p))


@pytest.mark.parametrize("n,k", [(3, 3), (64, 4), (300, 8), (683, 3)])
def test_with_layout_builder(ctxs, n, k):
    host, dev = ctxs
    p = graph_of(host, n, k)
    info, digests = compare(dev, p, layout=1)
    assert_built(info, digests, LAYOUT_STAGES)
    for name in ("rowmap", "woff", "wsplit", "pmap", "pidx"):
        assert digests[name] != FNV_BASIS, name
    s = host.debug_plan_layout_stats(p, 0, 1)
    for f in ("set_plan_builder", "set_multi_pair_builder", "set_multi_tile_builder", "set_layout_builder"):
        getattr(dev, f)(1)
    try:
        assert dev.debug_plan_layout_stats(p, 1, 1) == s
        assert triple(dev.plan_build_info()) == (1, 0, LAYOUT_STAGES)
    finally:
        for f in SWITCHES:
            getattr(dev, f)(0)


@pytest.fixture(scope="module")
def p200(ctxs):
    return graph_of(ctxs[0], 200, 4)


def edited(p, **kw):
    q = dataclasses.replace(p, **kw)
    assert q.validate()
    return q


def with_edges(p, rep):
    return edited(p, **{a: getattr(p, a)[rep] for a in EDGE_ARRAYS})


def out_edges_of_one_vertex(p, count):
    """the i columns of other vertices' edges of pair 0 rewritten to the copies of pair 0's first vertex until it has
    `count` out-edges in that pair"""
    ap = p.arap_pts.copy()
    pair0 = np.flatnonzero(p.arap_pair == 0)
    v = ap[pair0[0], :2].copy()
    have = int((ap[pair0, 0] == v[0]).sum())
    others = [e for e in pair0 if ap[e, 0] != v[0] and not set(ap[e, 2:]) & set(v)]
    for e in others[:count - have]:
        ap[e, :2] = v
    assert ((ap[:, 0] == v[0]) & (p.arap_pair == 0)).sum() == count
    return edited(p, arap_pts=ap)


# ---- edits of the (200, 4) graph that build_tiles_multi accepts -------------------------------------------------
def test_edges_not_pair_major(ctxs, p200):
    rep = np.random.default_rng(7).permutation(len(p200.arap_pts))
    q = with_edges(p200, rep)
    assert (np.diff(q.arap_pair) < 0).any()
    assert_built(*compare(ctxs[1], q))


def test_every_edge_doubled(ctxs, p200):
    assert_built(*compare(ctxs[1], with_edges(p200, np.repeat(np.arange(len(p200.arap_pts)), 2))))


def test_vertex_with_64_out_edges(ctxs, p200):
    assert_built(*compare(ctxs[1], out_edges_of_one_vertex(p200, 64)))


def test_all_keys_tie(ctxs, p200):
    pts = p200.points.copy()
    pts[:, :2] = (0.25, -0.5)
    assert_built(*compare(ctxs[1], edited(p200, points=pts)))


def test_without_order_xy(ctxs, p200):
    assert_built(*compare(ctxs[1], edited(p200, order_xy=None)))


def camera_points(p, cam):
    return np.unique(p.rep_point[p.rep_cam == cam])


def test_degenerate_and_signed_zero_boxes(ctxs, p200):
    """one camera's box has no extent in x, another's none in y; zeros of both signs in a third"""
    pts = p200.points.copy()
    pts[camera_points(p200, 0), 0] = 0.125
    pts[camera_points(p200, 2), 1] = -3.0
    sel = camera_points(p200, 3)
    pts[sel[::2], 0] = 0.0
    pts[sel[1::2], 0] = -0.0
    assert_built(*compare(ctxs[1], edited(p200, points=pts)))


# ---- edits that build_tiles_multi refuses: the device says so, the host says why ---------------------------------
def test_refused_vertex_with_65_out_edges(ctxs, p200):
    assert_refused(*compare(ctxs[1], out_edges_of_one_vertex(p200, 65)))


def test_refused_depth_edge_of_another_pair(ctxs, p200):
    s = p200.dep_scale.copy()
    s[0] = (s[0] + 2) % p200.n_scales
    assert_refused(*compare(ctxs[1], edited(p200, dep_scale=s)))


def test_refused_edge_moved_to_the_next_pair(ctxs, p200):
    pair = p200.arap_pair.copy()
    pair[0] = (pair[0] + 1) % p200.n_pairs
    assert_refused(*compare(ctxs[1], edited(p200, arap_pair=pair)))


def test_refused_copies_in_two_groups(ctxs, p200):
    ap = p200.arap_pts.copy()
    e = int(np.flatnonzero((ap[:, 0] != ap[0, 0]) & (ap[:, 0] != ap[0, 2]))[0])
    ap[0, 1] = ap[e, 1]                                 # another vertex's p2 copy
    assert_refused(*compare(ctxs[1], edited(p200, arap_pts=ap)))


def test_refused_point_without_edges(ctxs, p200):
    kw = dict(points=np.vstack([p200.points, [[0.01, 0.02, 0.3]]]))
    if p200.order_xy is not None:
        kw["order_xy"] = np.vstack([p200.order_xy, [[0.01, 0.02]]])
    q = edited(p200, **kw)
    assert q.n_points == p200.n_points + 1
    assert_refused(*compare(ctxs[1], q))


def test_edge_inside_one_group_is_refused_by_validation(ctxs, p200):
    ap = p200.arap_pts.copy()
    ap[0, 2:] = ap[0, :2]
    q = dataclasses.replace(p200, arap_pts=ap)
    dev = ctxs[1]
    for mode in (0, 1):
        dev.set_multi_pair_builder(mode)
        dev.set_multi_tile_builder(mode)
        try:
            with pytest.raises(capi.DeftriError) as e:
                dev.debug_plan_digest(q, mode, 1)
        finally:
            for f in SWITCHES:
                getattr(dev, f)(0)
        assert e.value.code == _abi.DEFTRI_E_ARG


def test_row_above_the_bound_builds_on_the_host(ctxs):
    """20 keyframes, all pairs: a row with 342 incidences, more than the 256 the per-run sort orders (kPlanRunMax)"""
    host, dev = ctxs
    p = graph_of(host, 60, 20)
    assert np.bincount(p.arap_pts.ravel(), minlength=p.n_points).max() > 256
    info, _ = compare(dev, p)
    assert triple(info) == (0, 2, 0), info


# ---- the switch and its neighbours --------------------------------------------------------------------------
def test_the_switch_alone(ctxs):
    host, dev = ctxs
    p = graph_of(host, 64, 4)
    info, _ = compare(dev, p, plan_builder=0)
    assert triple(info) == (0, 0, 0), info
    info, _ = compare(dev, p, multi=0, layout=1)
    assert triple(info) == (0, 1, 0), info
    info, _ = compare(dev, p, tile=0)
    assert triple(info) == (0, 1, 0), info
    # the one-pair tile builder does not reach several pairs
    info, _ = compare(dev, p, multi_tile=0, tile_builder=1)
    assert triple(info) == (1, 0, 0x3f), info


def test_one_pair_graph_is_as_before(ctxs):
    host, dev = ctxs
    m, _ = sim.simulate_two_view(n=300, seed=3, compact=True)
    one = host.build_graph(m, 1.0, 2e5, np.float32(0.003))
    assert one.n_pairs == 1
    info, digests = compare(dev, one)
    assert triple(info) == (1, 0, 0x3f), info
    assert digests["tile_trow"] == FNV_BASIS
    info, _ = compare(dev, one, tile_builder=1, layout=1)
    assert triple(info) == (1, 0, 0x1fff), info


def test_twice_on_one_context(ctxs):
    """the same graph before and after a smaller and a one-pair build: the arenas are reused, the result is the same"""
    host, dev = ctxs
    p, small = graph_of(host, 300, 8), graph_of(host, 4, 3)
    first, d1 = compare(dev, p, layout=1)
    assert triple(compare(dev, small, layout=1)[0]) == (1, 0, LAYOUT_STAGES)
    m, _ = sim.simulate_two_view(n=300, seed=3, compact=True)
    one = host.build_graph(m, 1.0, 2e5, np.float32(0.003))
    assert triple(compare(dev, one, layout=1, tile_builder=1)[0]) == (1, 0, 0x1fff)
    second, d2 = compare(dev, p, layout=1)
    assert triple(first) == triple(second) == (1, 0, LAYOUT_STAGES)
    assert d1 == d2


def test_both_layouts_share_one_tile_arena(ctxs):
    """one-pair and multi-pair builds in turn on a fresh context with all five switches on: both layouts are cut by one
    routine into one tile arena (a two-view graph of n correspondences has 2 n points: n = 257 and 65 here).
    The arena holds 8 bytes per padded entry (E <= entries <= 2 E + 64 tiles), 4 per edge for the order and 12 per cross
    slot (<= 2 E), and grows to 5/4 of what is asked.  It is allocated by the first build (two views of 257: 1,516
    edges, at most 225 KB asked, so at most 281 KB held).  (64, 4) asks at most 350 KB, so it holds at most 437 KB
    after it, grown or not.  Two views of 65 (366 edges) is the first graph's kind at a quarter of its size and runs in
    an arena left by another layout.  (300, 8) asks at least 12 bytes per edge of about 50,000, over 600 KB: it grows
    again.  A wrong capacity or a pointer into a freed arena shows as a digest that differs from the host's"""
    host = ctxs[0]

    def two_view(n):
        m, _ = sim.simulate_two_view(n=n, seed=3, compact=True)
        p = host.build_graph(m, 1.0, 2e5, np.float32(0.003))
        assert p.n_points == 2 * n and p.n_pairs == 1
        return p

    with capi.Context(0) as dev:
        for p, stages in ((two_view(257), 0x1fff), (graph_of(host, 64, 4), LAYOUT_STAGES), (two_view(65), 0x1fff),
                          (graph_of(host, 300, 8), LAYOUT_STAGES)):
            info, digests = compare(dev, p, layout=1, tile_builder=1)
            assert triple(info) == (1, 0, stages), info
            assert digests["tile_tab"] != FNV_BASIS
            assert (digests["tile_trow"] != FNV_BASIS) == (p.n_pairs > 1)


def test_upload_and_lm_solve_bit_for_bit(ctxs):
    """50,624 unknowns: the upload asks for the tile layout itself; pmap and pidx reach the solver on the device"""
    p = graph_of(ctxs[0], 2100, 8)
    assert p.n_unknowns == 50624
    out = []
    for mode in (0, 1):
        with capi.Context(0) as c:
            for f in ("set_plan_builder", "set_multi_pair_builder", "set_multi_tile_builder", "set_layout_builder"):
                getattr(c, f)(mode)
            c.set_linear_solver("pcg")
            c.upload(p)
            r = c.solve_lm(3)
            out.append((r, c.download(), c.plan_info(), c.plan_build_info()))
    (r0, s0, i0, b0), (r1, s1, i1, b1) = out
    assert i0 == i1 and i0["tiles"] > 0
    assert triple(b0) == (0, 0, 0)
    assert triple(b1) == (1, 0, LAYOUT_STAGES), b1
    for k in ("chi2_iter", "trials_iter", "lambda_final", "iterations", "pcg_iterations"):
        assert np.array_equal(np.asarray(r0[k]), np.asarray(r1[k])), k
    for a, b, what in zip(s0, s1, ("points", "scales", "T_g")):
        assert np.array_equal(a, b), what


def map_state(m):
    pos = np.array([mp.position for mp in m.map_points.values()])
    scales = np.array([kf.estimated_depth_scale for kf in m.keyframes.values()])
    tg = np.array([m.global_T[k].as7() for k in sorted(m.global_T)])
    return pos, scales, tg


def test_through_arap_optimization_twice():
    """the second call is the next round: the written-back points have moved, so graph and plan are rebuilt"""
    m, _ = sim.simulate_multi_view(n=2100, k=8)
    ma, mb = copy.deepcopy(m), copy.deepcopy(m)
    with capi.Context(0) as a, capi.Context(0) as b:
        for f in ("set_plan_builder", "set_multi_pair_builder", "set_multi_tile_builder", "set_layout_builder"):
            getattr(b, f)(1)
        before = map_state(ma)[0]
        for call in range(2):
            a.arap_optimization(ma, *W[:1], 50.0, W[1], 0.0, 0.0, W[2], 3)
            b.arap_optimization(mb, *W[:1], 50.0, W[1], 0.0, 0.0, W[2], 3)
            sa, sb = map_state(ma), map_state(mb)
            for x, y, what in zip(sa, sb, ("positions", "depth scales", "T_g")):
                assert np.array_equal(x, y), (call, what)
            assert not np.array_equal(sa[0], before)
            before = sa[0]
            assert triple(b.plan_build_info()) == (1, 0, LAYOUT_STAGES), (call, b.plan_build_info())
            assert a.plan_build_info()["builder_used"] == 0
