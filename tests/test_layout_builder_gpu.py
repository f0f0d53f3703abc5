"""deftri_set_layout_builder(1) on the device (csrc/plan_dev.hip): the plan's phase-1 blocks (dperm, blk,
hv_blk, hv_blk_off) and phase-2 wave layout (rowmap, woff, wsplit, pmap, pidx) built by kernels, against stages 7 and
8b of csrc/spcg_plan.cpp array by array (all 33 digests of deftri_debug_plan_digest), then through an upload — where
pmap and pidx reach the solver by a device-to-device copy — with an LM solve, and through the drop-in
arapOptimization call, bit for bit.

Sizes: own rows are 2 n, so 32 / 64 / 256 / 1024 correspondences end the rows on a wave, a sort window and several
windows exactly; about 43 correspondences fill the first ARAP block, 257 start the second depth block per scale.
deftri_debug_plan_layout_stats on the host build shows that an input holds the case it is here for."""
import copy
import dataclasses

import numpy as np
import pytest

from deftri import capi, sim

pytestmark = pytest.mark.gpu

W = (1.0, 2e5, np.float32(0.003))
FNV_BASIS = 1469598103934665603          # the digest of an empty array
ALL_STAGES, TILE_STAGES, PLAN_STAGES, ROW_STAGES = 0x1fff, 0x3ff, 0x3f, 0b111


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


def compare(dev, p, tile=1, plan_builder=1, tile_builder=1):
    """mode 0 against (plan builder 1, tile builder 1, layout builder 1) on one device context, all 33 digests;
    returns the build's info and the digests by name.  The switches are put back"""
    for f in (dev.set_plan_builder, dev.set_tile_builder, dev.set_layout_builder):
        f(0)
    names, want = dev.debug_plan_digest(p, 0, tile)
    info0 = dev.plan_build_info()
    assert (info0["builder_used"], info0["stages"], info0["reason"]) == (0, 0, 0)
    dev.set_tile_builder(tile_builder)
    dev.set_layout_builder(1)
    try:
        _, got = dev.debug_plan_digest(p, plan_builder, tile)
        info = dev.plan_build_info()
    finally:
        dev.set_tile_builder(0)
        dev.set_layout_builder(0)
    assert len(got) == 33
    for name, a, b in zip(names, want, got):
        assert a == b, f"{name} differs ({info})"
    return info, dict(zip(names, got))


def assert_built(info, stages=ALL_STAGES):
    assert (info["builder_used"], info["reason"], info["stages"]) == (1, 0, stages), info


@pytest.mark.parametrize("n", [3, 4, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 1023, 1024, 1025, 2049])
def test_two_view_graphs(ctxs, cloud, n):
    host, dev = ctxs
    p = graph_of(host, cloud, n)
    s = host.debug_plan_layout_stats(p, 0, 1)
    assert s["blocks"] - s["depth_blocks"] >= (2 if n >= 63 else 1)        # a full ARAP block and its tail
    assert s["depth_blocks"] >= (4 if n >= 257 else 2)                     # two scales; 257: a second block each
    if n >= 31:
        assert 0 < s["split_waves"] < s["waves"]
    info, digests = compare(dev, p)
    assert_built(info)
    for name in ("blk", "hv_blk", "dperm", "rowmap", "woff", "wsplit", "pmap", "pidx"):
        assert digests[name] != FNV_BASIS, name
    # the same figures from the device's arrays
    dev.set_plan_builder(1); dev.set_tile_builder(1); dev.set_layout_builder(1)
    try:
        assert dev.debug_plan_layout_stats(p, 1, 1) == s
        assert_built(dev.plan_build_info())
    finally:
        dev.set_plan_builder(0); dev.set_tile_builder(0); dev.set_layout_builder(0)


@pytest.fixture(scope="module")
def p300(ctxs, cloud):
    return graph_of(ctxs[0], cloud, 300)


def edited(p, **kw):
    q = dataclasses.replace(p, **kw)
    assert q.validate()
    return q


def test_sparse_graph_has_waves_without_steps(ctxs, p300):
    """300 more points that no edge touches (the unit-cap construction of the tile builder's test): rows without
    slots, and whole waves of them — zero steps, and they still exist"""
    rng = np.random.default_rng(5)
    lo, hi = p300.order_xy.min(0), p300.order_xy.max(0)
    xy = lo + (hi - lo) * rng.random((300, 2))
    q = edited(p300, points=np.vstack([p300.points, np.column_stack([xy, np.full(300, 0.3)])]),
               order_xy=np.vstack([p300.order_xy, xy]))
    s = ctxs[0].debug_plan_layout_stats(q, 0, 1)
    assert s["zero_step_waves"] > 0, s
    assert_built(compare(ctxs[1], q)[0])


def test_all_waves_split(ctxs, p300):
    """every ARAP edge listed twice: every row's count doubles, so every wave splits"""
    rep = np.repeat(np.arange(len(p300.arap_pts)), 2)
    q = edited(p300, arap_pts=p300.arap_pts[rep], arap_pair=p300.arap_pair[rep], arap_rot=p300.arap_rot[rep],
               arap_w=p300.arap_w[rep])
    s = ctxs[0].debug_plan_layout_stats(q, 0, 1)
    assert s["waves"] == s["split_waves"] > 0, s
    assert_built(compare(ctxs[1], q)[0])


def test_uneven_depth_edges(ctxs, p300):
    """a row with two depth edges and a row with none; all depth edges on scale 0; a problem of one scale"""
    dp = p300.dep_point.copy()
    assert dp[0] != dp[1]
    dp[1] = dp[0]
    assert_built(compare(ctxs[1], edited(p300, dep_point=dp))[0])
    zeros = np.zeros_like(p300.dep_scale)
    q = edited(p300, dep_scale=zeros)
    assert ctxs[0].debug_plan_layout_stats(q, 0, 1)["depth_blocks"] == 3          # 600 edges of one scale
    assert_built(compare(ctxs[1], q)[0])
    ones = np.ones_like(p300.dep_scale)
    assert_built(compare(ctxs[1], edited(p300, dep_scale=ones))[0])
    one = edited(p300, dep_scale=zeros, scales=p300.scales[:1])
    assert one.n_scales == 1
    assert_built(compare(ctxs[1], one)[0])


def test_5000_twice_on_one_context(ctxs, cloud):
    """the same graph before and after a smaller build: the arenas are reused, the result does not change"""
    host, dev = ctxs
    p, small = graph_of(host, cloud, 5000), graph_of(host, cloud, 64)
    first, d1 = compare(dev, p)
    assert_built(first)
    assert_built(compare(dev, small)[0])
    second, d2 = compare(dev, p)
    assert_built(second)
    assert d1 == d2


def test_refused_tile_layout_keeps_the_host_stages(ctxs, p300):
    """a vertex with 65 out-edges (the tile builder's test): build_tiles refuses, so the layout stages do not run"""
    ap = p300.arap_pts.copy()
    v = ap[0, :2].copy()
    have = int((ap[:, 0] == v[0]).sum())
    others = [e for e in range(len(ap)) if ap[e, 0] != v[0] and not set(ap[e, 2:]) & set(v)]
    for e in others[:65 - have]:
        ap[e, :2] = v
    assert (ap[:, 0] == v[0]).sum() == 65
    info, digests = compare(ctxs[1], edited(p300, arap_pts=ap))
    assert digests["tile_tab"] == FNV_BASIS
    assert_built(info, ROW_STAGES)


def test_not_applicable_eight_keyframes(ctxs):
    host, dev = ctxs
    p = host.build_graph(sim.multi_view_arrays(n=120, k=8), *W)
    assert p.n_pairs == 28
    info, _ = compare(dev, p)
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 1)


def test_not_applicable_without_the_tile_layout(ctxs, p300):
    info, _ = compare(ctxs[1], p300, tile=0)
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 1)


def test_no_effect_with_tile_builder_0(ctxs, p300):
    assert_built(compare(ctxs[1], p300, tile_builder=0)[0], PLAN_STAGES)


def test_no_effect_with_plan_builder_0(ctxs, p300):
    info, _ = compare(ctxs[1], p300, plan_builder=0)
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 0)


def test_layout_builder_0_keeps_the_tile_stages(ctxs, p300):
    dev = ctxs[1]
    dev.set_tile_builder(1)
    try:
        dev.debug_plan_digest(p300, 1, 1)
        assert_built(dev.plan_build_info(), TILE_STAGES)
    finally:
        dev.set_tile_builder(0)


@pytest.fixture(scope="module")
def scene20k():
    m, _ = sim.simulate_two_view(n=20000, seed=4, scale_scene=True, compact=True)
    return m


def test_upload_and_lm_solve_bit_for_bit(ctxs, scene20k):
    """the device-to-device hand-off of pmap and pidx: all three switches at 1 against all at 0"""
    p = ctxs[0].build_graph(scene20k, *W)
    assert p.n_unknowns >= 100000
    stats = ctxs[0].debug_plan_layout_stats(p, 0, 1)
    out = []
    for mode in (0, 1):
        with capi.Context(0) as c:
            c.set_plan_builder(mode)
            c.set_tile_builder(mode)
            c.set_layout_builder(mode)
            c.set_linear_solver("pcg")
            c.upload(p)
            r = c.solve_lm(5)
            out.append((r, c.download(), c.plan_info(), c.plan_build_info()))
    (r0, s0, i0, b0), (r1, s1, i1, b1) = out
    assert i0["plan"] == i1["plan"] and i0 == i1
    assert i1["phase1_blocks"] == stats["blocks"]
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
        b.set_layout_builder(1)
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
