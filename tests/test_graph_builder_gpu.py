"""deftri_set_graph_builder(1) on the device (csrc/graph_build_dev.hip): the CSR adjacency, the vector
map, the geometry, the slot scan, the point numbering and the edges built by the device stages against the host build
of a host-only context — every descriptor array and the point ids equal, and deftri_graph_build_info saying who
built.  The cases: one and several pairs, the smallest meshes and the block edges of the scans, null slots (the
slot-versus-position quirk), a non-identity vector map, ids outside the direct table, an input error, depth images,
the structure memo's next round on a device-built graph, and arapOptimization with all five builder switches on."""
import copy

import numpy as np
import pytest

from deftri import capi, sim
import depth_image_ref

pytestmark = pytest.mark.gpu

FIELDS = ("points", "tg", "scales", "cam_kb8", "cam_pose", "rep_point", "rep_cam", "rep_obs", "rep_info",
          "dep_point", "dep_scale", "dep_cam", "dep_meas", "dep_info", "arap_pts", "arap_pair", "arap_rot",
          "arap_w", "rot", "pair_area", "pair_info", "order_xy", "point_ids")
W = (1.0, 2e5, np.float32(0.003))
W_MULTI = (1.0, 1e7, np.float32(0.3))
FULL = 0x3f


class Edited:
    """A map whose C view is edited before every call: edit(mc, keep) changes the arrays of keep["arrays"] — per
    keyframe in map order (key, point_id, point_pos, obs_index, kp_uv, kp_octave, depth, ...) — in place."""

    def __init__(self, m, edit):
        self.m, self.edit = m, edit

    def to_c(self):
        mc, keep = self.m.to_c()
        self.edit(mc, keep)
        return mc, keep


def assert_equal(want, got):
    for f in FIELDS:
        assert np.array_equal(getattr(want, f), getattr(got, f)), f


def assert_built(info):
    assert (info["builder_used"], info["stages"], info["reason"]) == (1, FULL, 0), info
    assert info["ms"] > 0


def host_graph(m, w=W, pair_window=0):
    with capi.Context(-1) as h:
        if pair_window:
            h.set_pair_window(pair_window)
        return h.build_graph(m, *w)


def device_graph(m, w=W, pair_window=0, mesh_builder=0):
    """(graph, info) of a new device context with graph builder 1"""
    with capi.Context(0) as d:
        d.set_graph_builder(1)
        d.set_mesh_builder(mesh_builder)
        if pair_window:
            d.set_pair_window(pair_window)
        return d.build_graph(m, *w), d.graph_build_info()


# ---- the scenes (each with its numpy preconditions, checked before any build) ----
def two_view(n, seed):
    return sim.simulate_two_view(n=n, seed=seed, scale_scene=True, compact=True)[0]


@pytest.fixture(scope="module")
def scene3000():
    return two_view(3000, 1)


def prefix_scene(cloud, n):
    """The first n correspondences of a compacted cloud: a scene of exactly n points per keyframe."""
    orig, moved = cloud
    m, gt = sim.simulate_two_view(orig=orig[:n], moved=moved[:n], compact=True)
    assert len(gt["original"]) == n and gt["valid"].all()
    return m


def make_cloud():
    _, gt = sim.simulate_two_view(n=400, seed=11, compact=True)
    assert len(gt["original"]) >= 257
    return gt["original"], gt["moved"]


@pytest.fixture(scope="module")
def cloud():
    return make_cloud()


def null_slot_scene(n, seed, slots):
    """tests/test_graph.py::test_null_slot_quirk's recipe: the correspondences at `slots` dropped in both keyframes"""
    m, _ = sim.simulate_two_view(n=n, seed=seed)
    kf0, kf1 = m.keyframes[0], m.keyframes[1]
    for s in slots:
        for kf in (kf0, kf1):
            mp = kf.map_points[s]
            assert mp is not None
            kf.map_points[s] = None
            m.kf_obs[kf.id].pop(mp.id, None)
    return m


def squeeze_null_slots(mc, keep):
    """The compacted scene of a map with null slots: every keyframe's slots without the null ones."""
    for n, arrays in enumerate(keep["arrays"]):
        pid, pos, obs = arrays[1], arrays[2], arrays[3]
        ok = pid >= 0
        pid2, pos2, obs2 = np.ascontiguousarray(pid[ok]), np.ascontiguousarray(pos[ok]), np.ascontiguousarray(obs[ok])
        c = mc.keyframes[n]
        c.n_slots = int(ok.sum())
        c.point_id = pid2.ctypes.data_as(type(c.point_id))
        c.point_pos = pos2.ctypes.data_as(type(c.point_pos))
        c.obs_index = obs2.ctypes.data_as(type(c.obs_index))
        keep.setdefault("squeezed", []).append((pid2, pos2, obs2))


def null_slots_3000():
    rng = np.random.default_rng(17)
    m0, _ = sim.simulate_two_view(n=3000, seed=5)
    full = [s for s in range(3000) if m0.keyframes[0].map_points[s] is not None and m0.keyframes[1].map_points[s] is not None]
    slots = sorted(int(s) for s in rng.choice(full, size=30, replace=False))
    return null_slot_scene(3000, 5, slots)


NEAR_DUPLICATES = ((100, 2200), (1501, 7), (2999, 1500))      # (slot moved, slot whose position it takes)


def near_duplicate_edit(mc, keep):
    """three slots of the pair's keyframe 1 (the later keyframe in map order) one fp32 ulp in x from another slot"""
    pos = keep["arrays"][1][2]
    for s, t in NEAR_DUPLICATES:
        pos[s] = pos[t]
        pos[s, 0] = np.nextafter(pos[t, 0], np.float32(np.inf))


def check_near_duplicates(m):
    """numpy precondition: each pair is distinct in fp64 and satisfies Eigen's isApprox(1e-6), so the host's vector
    map is not the identity"""
    _, keep = Edited(m, near_duplicate_edit).to_c()
    pos = keep["arrays"][1][2].astype(np.float64)
    assert len(pos) >= 3000 and (keep["arrays"][1][1] >= 0).all()
    for s, t in NEAR_DUPLICATES:
        v, p = pos[s], pos[t]
        assert not np.array_equal(v, p)
        assert ((v - p) ** 2).sum() <= 1e-12 * min((v * v).sum(), (p * p).sum())


def same_xy_edit(mc, keep):
    """one slot of keyframe 1 straight above another: the triangulation skips one of the two"""
    pos = keep["arrays"][1][2]
    pos[1200, :2] = pos[40, :2]
    assert pos[1200, 2] != pos[40, 2]


def spread_ids(mc, keep):
    for arrays in keep["arrays"]:
        pid = arrays[1]
        pid[pid >= 0] *= 1000


def check_spread_ids(m):
    _, keep = Edited(m, spread_ids).to_c()
    ids = np.concatenate([a[1][a[1] >= 0] for a in keep["arrays"]])
    assert ids.max() - ids.min() + 1 > max(4 * len(ids), 65536)


BAD_SLOT = 7


def bad_observation(mc, keep):
    """one obs_index one past the end of its keyframe's observations"""
    arrays = keep["arrays"][0]
    assert arrays[1][BAD_SLOT] >= 0 and keep["arrays"][1][1][BAD_SLOT] >= 0 and arrays[3][BAD_SLOT] >= 0
    arrays[3][BAD_SLOT] = mc.keyframes[0].n_obs


NEXT_ROUND_AMPLITUDE = 1e-6     # metres: the host context answers the moved map from the structure memo


def next_round_edit(mc, keep):
    rng = np.random.default_rng(23)
    for arrays in keep["arrays"]:
        pos = arrays[2]
        pos += rng.normal(0, NEXT_ROUND_AMPLITUDE, pos.shape).astype(np.float32)


def next_round_host(m):
    """the host context's two builds; the second a structure-memo hit"""
    with capi.Context(-1) as h:
        h.build_graph(m, *W)
        p = h.build_graph(Edited(m, next_round_edit), *W)
        assert h.graph_stats()[:2] == (0, 1)
        return p


# ---- the cases ----
@pytest.mark.parametrize("mesh_builder", [0, 1])
@pytest.mark.parametrize("n,seed", [(3000, 1), (20000, 2)])
def test_two_view(n, seed, mesh_builder):
    m = two_view(n, seed)
    got, info = device_graph(m, mesh_builder=mesh_builder)
    assert_equal(host_graph(m), got)
    assert_built(info)


@pytest.mark.parametrize("n", [3, 4, 255, 256, 257])
def test_smallest_meshes(cloud, n):
    m = prefix_scene(cloud, n)
    want = host_graph(m)
    assert want.n_points == 2 * n
    got, info = device_graph(m)
    assert_equal(want, got)
    assert_built(info)


@pytest.mark.parametrize("which", ["200", "3000"])
def test_null_slots(which):
    m = null_slot_scene(200, 5, (3, 40, 41, 150)) if which == "200" else null_slots_3000()
    want = host_graph(m)
    got, info = device_graph(m)
    assert_equal(want, got)
    assert_built(info)
    # the slot-versus-position quirk ran: the squeezed scene has other ARAP edges
    assert not np.array_equal(got.arap_pts, host_graph(Edited(m, squeeze_null_slots)).arap_pts)


def test_near_duplicates(scene3000):
    check_near_duplicates(scene3000)
    m = Edited(scene3000, near_duplicate_edit)
    got, info = device_graph(m)
    assert_equal(host_graph(m), got)
    assert info["reason"] in (0, 3), info
    assert info["builder_used"] == (1 if info["reason"] == 0 else 0)


def test_a_mesh_that_skips_a_point(scene3000):
    """not applicable: the host build runs, from the triangulation the device path had made"""
    m = Edited(scene3000, same_xy_edit)
    got, info = device_graph(m)
    assert_equal(host_graph(m), got)
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 1)


@pytest.mark.parametrize("pair_window", [0, 1])
def test_several_pairs(pair_window):
    m = sim.multi_view_arrays(n=2000, k=5, seed=3)
    want = host_graph(m, W_MULTI, pair_window)
    assert want.n_pairs == (4 if pair_window else 10)
    got, info = device_graph(m, W_MULTI, pair_window)
    assert_equal(want, got)
    assert_built(info)


def test_ids_outside_the_direct_table():
    m0, _ = sim.simulate_two_view(n=400, seed=3)
    check_spread_ids(m0)
    m = Edited(m0, spread_ids)
    got, info = device_graph(m)
    assert_equal(host_graph(m), got)
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 1)


def test_input_error():
    m, _ = sim.simulate_two_view(n=400, seed=3)
    bad = Edited(m, bad_observation)
    with capi.Context(-1) as h, capi.Context(0) as d:
        d.set_graph_builder(1)
        with pytest.raises(capi.DeftriError) as eh:
            h.build_graph(bad, *W)
        with pytest.raises(capi.DeftriError) as ed:
            d.build_graph(bad, *W)
        assert eh.value.code == ed.value.code and str(eh.value) == str(ed.value)
        info = d.graph_build_info()
        assert (info["builder_used"], info["reason"]) == (0, 2)
        got = d.build_graph(m, *W)
        assert_equal(h.build_graph(m, *W), got)
        assert_built(d.graph_build_info())


def test_depth_images():
    m, _ = sim.simulate_two_view(n=300, seed=3)
    m = depth_image_ref.synthetic_images(m, (560, 640), seed=7)
    want = host_graph(m)
    got, info = device_graph(m)
    assert_equal(want, got)
    assert np.array_equal(want.dep_meas.view(np.uint64), got.dep_meas.view(np.uint64))
    assert_built(info)


def test_next_round(scene3000):
    want = next_round_host(scene3000)
    with capi.Context(0) as d:
        d.set_graph_builder(1)
        d.build_graph(scene3000, *W)
        first = d.graph_build_info()
        assert_built(first)
        got = d.build_graph(Edited(scene3000, next_round_edit), *W)
        assert d.graph_stats()[:2] == (0, 1)
        assert d.graph_build_info() == first        # a memo hit leaves the info of the last full build
    assert_equal(want, got)


def map_state(m):
    pos = np.array([mp.position for mp in m.map_points.values()])
    scales = np.array([kf.estimated_depth_scale for kf in m.keyframes.values()])
    tg = np.array([m.global_T[k].as7() for k in sorted(m.global_T)])
    return pos, scales, tg


def test_end_to_end(scene3000):
    ma, mb = copy.deepcopy(scene3000), copy.deepcopy(scene3000)
    with capi.Context(0) as a, capi.Context(0) as b:
        for f in (b.set_mesh_builder, b.set_plan_builder, b.set_tile_builder, b.set_layout_builder, b.set_graph_builder):
            f(1)
        a.arap_optimization(ma, 1.0, 50.0, 2e5, 0.0, 0.0, np.float32(0.003), 3)
        b.arap_optimization(mb, 1.0, 50.0, 2e5, 0.0, 0.0, np.float32(0.003), 3)
        assert_built(b.graph_build_info())
        assert a.graph_build_info()["builder_used"] == 0
    sa, sb = map_state(ma), map_state(mb)
    assert not np.array_equal(sa[0], map_state(scene3000)[0])
    for x, y, what in zip(sa, sb, ("positions", "depth scales", "T_g")):
        assert np.array_equal(x, y), what
