"""deftri_set_multi_pair_builder(1) on the device (csrc/plan_dev.hip): the tile plan of several keyframe
pairs — groups, Morton order, the keyframe-major rows, rotation numbering, edges by row, incidences, and with layout
builder 1 the wave layout — built by kernels, against the host passes of csrc/spcg_plan.cpp array by array (all 33
digests of deftri_debug_plan_digest), then through an upload with an LM solve and through the drop-in arapOptimization
call, bit for bit.

Sizes: P = n k points.  The radix sort's workgroup holds 256 keys (P = 255, 256, 258), the multi-block scan's tile 2048
elements (P = 2048, 2049); k = 8 gives 28 pairs, 56 scales and 8 cameras, the window of 2 over 20 keyframes 37 pairs.

Not here: non-finite points.  Problem.validate() admits them, but the library's own validation refuses such a
descriptor before any plan is built (test_non_finite_points_are_refused), so neither build sees one."""
import copy
import dataclasses

import numpy as np
import pytest

from deftri import _abi, capi, sim

pytestmark = pytest.mark.gpu

W = (1.0, 1e7, np.float32(0.3))
FNV_BASIS = 1469598103934665603          # the digest of an empty array
PLAN_STAGES, LAYOUT_STAGES, ROW_STAGES = 0x3f, 0x183f, 0b111
SWITCHES = ("set_plan_builder", "set_tile_builder", "set_layout_builder", "set_multi_pair_builder")


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


def compare(dev, p, tile=1, plan_builder=1, multi=1, layout=0, tile_builder=0):
    """mode 0 against plan builder 1 with the multi-pair builder (and the others as given) on one device context, all
    33 digests; returns the build's info and the digests by name.  The switches are put back"""
    for f in SWITCHES:
        getattr(dev, f)(0)
    names, want = dev.debug_plan_digest(p, 0, tile)
    info0 = dev.plan_build_info()
    assert (info0["builder_used"], info0["stages"], info0["reason"]) == (0, 0, 0)
    dev.set_multi_pair_builder(multi)
    dev.set_layout_builder(layout)
    dev.set_tile_builder(tile_builder)
    try:
        _, got = dev.debug_plan_digest(p, plan_builder, tile)
        info = dev.plan_build_info()
    finally:
        for f in SWITCHES:
            getattr(dev, f)(0)
    assert len(got) == 33
    for name, a, b in zip(names, want, got):
        assert a == b, f"{name} differs ({info})"
    return info, dict(zip(names, got))


def triple(info):
    return info["builder_used"], info["reason"], info["stages"]


def assert_built(info, digests, stages=PLAN_STAGES):
    """the device build; where build_tiles_multi refused the graph, the device's rows and the host's rest"""
    want = ROW_STAGES if digests["tile_tab"] == FNV_BASIS else stages
    assert triple(info) == (1, 0, want), info


@pytest.mark.parametrize("n,k", [(3, 3), (4, 3), (85, 3), (64, 4), (86, 3), (512, 4), (683, 3), (1025, 3), (300, 8)])
def test_all_pairs_graphs(ctxs, n, k):
    host, dev = ctxs
    info, digests = compare(dev, graph_of(host, n, k))
    assert digests["tile_tab"] != FNV_BASIS               # build_tiles_multi accepts every one of these graphs
    assert triple(info) == (1, 0, PLAN_STAGES), info


def test_windowed_graph(ctxs):
    host, dev = ctxs
    host.set_pair_window(2)
    try:
        p = host.build_graph(sim.multi_view_arrays(n=120, k=20), *W)
    finally:
        host.set_pair_window(0)
    assert p.n_pairs == 37 and p.n_scales == 74
    info, digests = compare(dev, p)
    assert digests["tile_tab"] != FNV_BASIS
    assert triple(info) == (1, 0, PLAN_STAGES), info


@pytest.mark.parametrize("n,k", [(3, 3), (64, 4), (300, 8), (683, 3)])
def test_with_layout_builder(ctxs, n, k):
    host, dev = ctxs
    p = graph_of(host, n, k)
    info, digests = compare(dev, p, layout=1)
    assert triple(info) == (1, 0, LAYOUT_STAGES), info
    for name in ("rowmap", "woff", "wsplit", "pmap", "pidx"):
        assert digests[name] != FNV_BASIS, name
    s = host.debug_plan_layout_stats(p, 0, 1)
    dev.set_plan_builder(1); dev.set_multi_pair_builder(1); dev.set_layout_builder(1)
    try:
        assert dev.debug_plan_layout_stats(p, 1, 1) == s
        assert triple(dev.plan_build_info()) == (1, 0, LAYOUT_STAGES)
    finally:
        for f in SWITCHES:
            getattr(dev, f)(0)


def test_tile_builder_has_no_effect(ctxs):
    host, dev = ctxs
    info, _ = compare(dev, graph_of(host, 64, 4), tile_builder=1, layout=1)
    assert triple(info) == (1, 0, LAYOUT_STAGES), info


@pytest.fixture(scope="module")
def p200(ctxs):
    return graph_of(ctxs[0], 200, 4)


def edited(p, **kw):
    q = dataclasses.replace(p, **kw)
    assert q.validate()
    return q


def test_one_edge_names_another_camera(ctxs, p200):
    """the first reprojection edge's camera changed: its point's other edges still name the old one, so one_cam is
    false and the rows fall back to the groups' order"""
    cam = p200.rep_cam.copy()
    cam[0] = (cam[0] + 1) % len(p200.cam_pose)
    assert_built(*compare(ctxs[1], edited(p200, rep_cam=cam)))


def test_a_point_with_two_cameras_keeps_the_group_order(ctxs, p200):
    """two reprojection edges at one point that name different cameras: one_cam is false, the rows are the groups'"""
    e = int(np.flatnonzero(p200.rep_cam != p200.rep_cam[0])[0])
    point = p200.rep_point.copy()
    point[e] = point[0]
    q = edited(p200, rep_point=point)
    assert len({(a, b) for a, b in zip(q.rep_point, q.rep_cam) if a == point[0]}) == 2
    assert_built(*compare(ctxs[1], q))
    # and with the later edge first in edge order
    point = p200.rep_point.copy()
    point[0] = point[e]
    assert_built(*compare(ctxs[1], edited(p200, rep_point=point)))


def camera_points(p, cam):
    return np.unique(p.rep_point[p.rep_cam == cam])


def test_all_keys_of_one_camera_tie(ctxs, p200):
    pts = p200.points.copy()
    sel = camera_points(p200, 1)
    assert len(sel) == 200
    pts[sel, :2] = (0.25, -0.5)
    assert_built(*compare(ctxs[1], edited(p200, points=pts)))


def test_degenerate_camera_box(ctxs, p200):
    """one camera's box has no extent in x, another's none in y; zeros of both signs in a third"""
    pts = p200.points.copy()
    pts[camera_points(p200, 0), 0] = 0.125
    pts[camera_points(p200, 2), 1] = -3.0
    sel = camera_points(p200, 3)
    pts[sel[::2], 0] = 0.0
    pts[sel[1::2], 0] = -0.0
    assert_built(*compare(ctxs[1], edited(p200, points=pts)))


def test_point_without_edges_is_refused_by_the_tile_layout(ctxs, p200):
    """a point no edge touches is the bucket past the last camera, and a row in no pair's mesh: build_tiles_multi
    refuses, and the host goes on from the device's rows"""
    kw = dict(points=np.vstack([p200.points, [[0.01, 0.02, 0.3]]]))
    if p200.order_xy is not None:
        kw["order_xy"] = np.vstack([p200.order_xy, [[0.01, 0.02]]])
    q = edited(p200, **kw)
    assert q.n_points == p200.n_points + 1
    info, digests = compare(ctxs[1], q)
    assert digests["tile_tab"] == FNV_BASIS
    assert triple(info) == (1, 0, ROW_STAGES), info


def test_without_order_xy(ctxs, p200):
    assert_built(*compare(ctxs[1], edited(p200, order_xy=None)))
    xy = np.random.default_rng(3).random((p200.n_points, 2))
    assert_built(*compare(ctxs[1], edited(p200, order_xy=xy)))


def test_non_finite_points_are_refused(ctxs, p200):
    pts = p200.points.copy()
    pts[5, 0] = np.nan
    pts[9, 1] = np.inf
    dev = ctxs[1]
    for mode in (0, 1):
        with pytest.raises(capi.DeftriError) as e:
            dev.debug_plan_digest(edited(p200, points=pts), mode, 1)
        assert e.value.code == _abi.DEFTRI_E_ARG


def test_row_above_the_bound_builds_on_the_host(ctxs):
    """20 keyframes, all pairs: a row with 342 incidences, more than the 256 the per-run sort orders (kPlanRunMax)"""
    host, dev = ctxs
    p = graph_of(host, 60, 20)
    inc = np.bincount(p.arap_pts.ravel(), minlength=p.n_points)
    assert inc.max() > 256
    info, _ = compare(dev, p)
    assert triple(info) == (0, 2, 0), info


def test_the_switch_alone(ctxs):
    host, dev = ctxs
    p = graph_of(host, 64, 4)
    info, _ = compare(dev, p, plan_builder=0)
    assert triple(info) == (0, 0, 0), info
    info, _ = compare(dev, p, multi=0, layout=1)
    assert triple(info) == (0, 1, 0), info
    info, _ = compare(dev, p, tile=0)
    assert triple(info) == (0, 1, 0), info


def test_twice_on_one_context(ctxs):
    """the same graph before and after a smaller and a one-pair build: the arena is reused, the result is the same"""
    host, dev = ctxs
    p, small = graph_of(host, 300, 8), graph_of(host, 4, 3)
    first, d1 = compare(dev, p, layout=1)
    assert triple(compare(dev, small, layout=1)[0]) == (1, 0, LAYOUT_STAGES)
    m, _ = sim.simulate_two_view(n=300, seed=3, compact=True)
    one = host.build_graph(m, 1.0, 2e5, np.float32(0.003))
    assert one.n_pairs == 1
    assert compare(dev, one, layout=1, tile_builder=1)[0]["builder_used"] == 1
    second, d2 = compare(dev, p, layout=1)
    assert triple(first) == triple(second) == (1, 0, LAYOUT_STAGES)
    assert d1 == d2


def test_upload_and_lm_solve_bit_for_bit(ctxs):
    """50,624 unknowns: the upload asks for the tile layout itself; pmap and pidx reach the solver on the device"""
    p = graph_of(ctxs[0], 2100, 8)
    assert p.n_unknowns == 50624
    out = []
    for mode in (0, 1):
        with capi.Context(0) as c:
            c.set_plan_builder(mode)
            c.set_multi_pair_builder(mode)
            c.set_layout_builder(mode)
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
        b.set_plan_builder(1)
        b.set_multi_pair_builder(1)
        b.set_layout_builder(1)
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
