"""deftri_set_plan_builder(1) on the device (csrc/plan_dev.hip): the one-pair tile plan's groups, Morton
order, rows, rotation numbering, edges by row and incidences built by kernels, against the host passes of
csrc/spcg_plan.cpp array by array (deftri_debug_plan_digest), then through an upload with an LM solve and through the
drop-in arapOptimization call, bit for bit.

Sizes: the radix sort's workgroup holds 256 groups (one group per correspondence: 255, 256, 257), the multi-block
scan's 2048 elements; its scans run over P + 1 = 2 n + 1 flags and counts (n = 1023: 2047, n = 1024: 2049) and over the
radix sort's 128 x ceil(P / 256) digit counts (n = 2048: 2048 exactly, n = 2047 / 2049: one tile less / more)."""
import copy
import dataclasses

import numpy as np
import pytest

from deftri import capi, sim

pytestmark = pytest.mark.gpu

W = (1.0, 2e5, np.float32(0.003))
FNV_BASIS = 1469598103934665603          # the digest of an empty array
ALL_STAGES, ROW_STAGES = 0b111111, 0b000111


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


def compare(dev, p, tile=1, refused_ok=False):
    """mode 1 against mode 0 on one device context, array by array; returns the build's info"""
    names, want = dev.debug_plan_digest(p, 0, tile)
    info0 = dev.plan_build_info()
    assert (info0["builder_used"], info0["stages"], info0["reason"]) == (0, 0, 0)
    _, got = dev.debug_plan_digest(p, 1, tile)
    info = dev.plan_build_info()
    for name, a, b in zip(names, want, got):
        assert a == b, f"{name} differs ({info})"
    digests = dict(zip(names, got))
    if refused_ok and digests["tile_tab"] == FNV_BASIS:
        info["expected_stages"] = ROW_STAGES          # build_tiles refused: the rest was built on the host
    else:
        info["expected_stages"] = ALL_STAGES
    return info


def assert_device_built(info):
    assert info["builder_used"] == 1 and info["reason"] == 0 and info["stages"] == info["expected_stages"], info


@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 2047, 2048, 2049, 5000])
def test_two_view_graphs(ctxs, cloud, n):
    host, dev = ctxs
    info = compare(dev, graph_of(host, cloud, n))
    assert info["builder_used"] == 1 and info["reason"] == 0 and info["stages"] == ALL_STAGES, info


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


def test_all_keys_tie(ctxs, p300):
    assert_device_built(compare(ctxs[1], edited(p300, order_xy=np.full_like(p300.order_xy, 0.25)), refused_ok=True))


def test_nan_and_inf_coordinates(ctxs, p300):
    xy = p300.order_xy.copy()
    a = p300.arap_pts[0]
    xy[min(a[0], a[1]), 0] = np.nan                  # the representatives (smallest ids) of edge 0's two groups
    xy[min(a[2], a[3]), 1] = np.inf
    xy[p300.n_points - 1] = (-np.inf, np.nan)
    assert_device_built(compare(ctxs[1], edited(p300, order_xy=xy), refused_ok=True))


def test_without_order_xy(ctxs, p300):
    assert_device_built(compare(ctxs[1], edited(p300, order_xy=None), refused_ok=True))


def test_singleton_group(ctxs, p300):
    """a point no ARAP edge touches: a group of its own, a row without incidences or edges"""
    q = edited(p300, points=np.vstack([p300.points, [[0.01, 0.02, 0.3]]]), order_xy=np.vstack([p300.order_xy, [[0.01, 0.02]]]))
    assert q.n_points == p300.n_points + 1
    assert_device_built(compare(ctxs[1], q, refused_ok=True))


def test_chain_and_large_group(ctxs, p300):
    """the union pairs (columns 0, 1) of some edges rewritten: four links chain five points in descending order (the
    roots are re-linked at every step; with their keyframe copies a group of 10), 34 links join 35 vertices' copies
    into one group of 70 points (more than a wave, and a run of 70 in the row sort)"""
    ap = p300.arap_pts.copy()
    firsts = np.unique(ap[:, 0])                      # one copy of every vertex
    chain = firsts[-5:][::-1]
    big = firsts[:70:2][:35]
    relink(ap, [(chain[k], chain[k + 1]) for k in range(4)] + [(big[k + 1], big[0]) for k in range(34)])
    assert_device_built(compare(ctxs[1], edited(p300, arap_pts=ap), refused_ok=True))


def test_run_above_the_bound_builds_on_the_host(ctxs, p300):
    """129 links join 130 vertices' copies into one group of 260 points: a run of the row sort longer than the 256
    its per-run sort orders (kPlanRunMax), so the kernel marks the build and the whole plan is the host's"""
    ap = p300.arap_pts.copy()
    firsts = np.unique(ap[:, 0])
    relink(ap, [(firsts[k + 1], firsts[0]) for k in range(129)])
    info = compare(ctxs[1], edited(p300, arap_pts=ap))
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 2), info


def test_not_applicable_eight_keyframes(ctxs):
    host, dev = ctxs
    p = host.build_graph(sim.multi_view_arrays(n=120, k=8), *W)
    assert p.n_pairs == 28
    info = compare(dev, p)
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 1)


def test_not_applicable_without_the_tile_layout(ctxs, p300):
    info = compare(ctxs[1], p300, tile=0)
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 1)


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
            c.set_linear_solver("pcg")
            c.upload(p)
            r = c.solve_lm(5)
            out.append((r, c.download(), c.plan_info(), c.plan_build_info()))
    (r0, s0, i0, b0), (r1, s1, i1, b1) = out
    assert i0["plan"] == i1["plan"] and i0 == i1
    assert b0["builder_used"] == 0 and b0["reason"] == 0
    assert b1["builder_used"] == 1 and b1["reason"] == 0 and b1["stages"] == ALL_STAGES, b1
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
        before = map_state(ma)[0]
        for call in range(2):
            a.arap_optimization(ma, 1.0, 50.0, 2e5, 0.0, 0.0, np.float32(0.003), 3)
            b.arap_optimization(mb, 1.0, 50.0, 2e5, 0.0, 0.0, np.float32(0.003), 3)
            sa, sb = map_state(ma), map_state(mb)
            for x, y, what in zip(sa, sb, ("positions", "depth scales", "T_g")):
                assert np.array_equal(x, y), (call, what)
            assert not np.array_equal(sa[0], before)
            before = sa[0]
            info = b.plan_build_info()
            assert info["builder_used"] == 1 and info["stages"] == ALL_STAGES and info["reason"] == 0, (call, info)
            assert a.plan_build_info()["builder_used"] == 0
