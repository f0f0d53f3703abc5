"""guidedMatching, searchWithProjection and Map::updateOrientationAndDescriptor on a host-only context (the
library's sequential loops) against the numpy restatements of deftri.matching: the reference's quirks one by
one, the order dependence of the claims, and the ABI.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from deftri import _abi, capi, matching
from deftri.mapmodel import KeyFrame, Map, MapPoint
from deftri.sim import inv_sigma2_table
import matching_scenes as ms
import projection_scenes as ps


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


def run(host, s):
    """The host-only context's result, checked against the fp32 restatement."""
    g, r = host.search_with_projection(*ps.args(s)), ps.ref(s)
    for k in ("match", "status", "predicted_octave", "best", "second", "slot_point"):
        np.testing.assert_array_equal(getattr(g, k), r[k], err_msg=k)
    for k, v in r["report"].items():
        assert g.report[k] == v, k
    assert g.report["rounds"] == 1 and g.report["round_trips"] == 0
    return g


def test_clamp_to_n_scales_is_undefined(host):
    g = run(host, ps.point_scene(0.8, 7.5, [(0.5, 0.5, 7, 2)]))           # min_dist = max / 1.2^7 > dist: status 2
    assert g.status[0] == matching.INV_DIST and g.predicted_octave[0] == -1
    s = ps.point_scene(0.8, 7.5, [(0.5, 0.5, 7, 2)])
    s["min_dist"] = s["max_dist"] / np.float32(10.0)
    g = run(host, s)
    assert g.status[0] == matching.UNDEFINED and g.predicted_octave[0] == ps.N_SCALES and g.match[0] == -1
    assert g.report["n_undefined"] == 1 and (g.slot_point == -1).all()
    s = ps.point_scene(0.8, 6.5, [(0.5, 0.5, 7, 2)])                       # the last defined octave is searched
    g = run(host, s)
    assert g.status[0] == matching.MATCHED and g.predicted_octave[0] == ps.N_SCALES - 1


def test_radius_switch_at_0_998(host):
    keys = [(3.0, 1.0, 3, 2)]                                              # inside 4.0, outside 2.5 scale factors
    wide = run(host, ps.point_scene(0.99, 2.5, keys))
    narrow = run(host, ps.point_scene(0.9995, 2.5, keys))
    assert wide.status[0] == matching.MATCHED and narrow.status[0] == matching.NO_CANDIDATES
    assert narrow.report["n_no_candidates"] == 1


def test_occupied_slot_is_skipped_entirely(host):
    keys = [(0.5, 0.5, 3, 1), (-0.5, 0.5, 3, 10), (0.5, -0.5, 3, 40)]
    g = run(host, ps.point_scene(0.8, 2.5, keys, slot=[-2, -1, -1]))
    assert (g.match[0], g.best[0], g.second[0]) == (1, 10, 40)            # 1 is neither best nor second
    np.testing.assert_array_equal(g.slot_point, [-2, 0, -1])
    g = run(host, ps.point_scene(0.8, 2.5, keys[:1], slot=[-2]))          # a candidate, but occupied: rejected, not status 3
    assert g.status[0] == matching.REJECTED and (g.best[0], g.second[0]) == (255, 255)


def test_tie_for_best_rejects(host):
    s = ps.point_scene(0.8, 2.5, [(0.5, 0.5, 3, 4), (-0.5, 0.5, 3, 4)])
    s["desc2"][1] = ms.flip_bits(np.zeros(32, np.uint8), [100, 101, 102, 103])
    g = run(host, s)
    assert g.status[0] == matching.REJECTED and (g.best[0], g.second[0]) == (4, 4)


@pytest.mark.parametrize("first", [0, 1])
def test_order_dependence(host, first):
    """Two map points on one lone keypoint: the first takes it, the second finds it occupied."""
    g = run(host, ps.point_scene(0.8, 2.5, [(0.5, 0.5, 3, 3)], n_points=2, descs=[first, 1 - first]))
    np.testing.assert_array_equal(g.match, [0, -1])
    np.testing.assert_array_equal(g.status, [matching.MATCHED, matching.REJECTED])
    np.testing.assert_array_equal(g.slot_point, [0])
    assert g.best[0] == 3 - first and g.best[1] == 255


def test_chain_takes_the_keypoint_the_previous_point_left(host):
    s = ps.chain_scene()
    g = run(host, s)
    np.testing.assert_array_equal(g.match, s["expect"])
    assert (g.status == matching.MATCHED).all() and len(s["expect"]) >= 8


def guided_args(s, has, octave1, wsf):
    return (s["grid"], s["Tcw"], s["kb8"], s["uv2"], s["octave2"], s["desc2"], has, s["pos"], octave1, s["desc"], s["th"], wsf)


def test_guided_integer_window(host):
    """radius = float(15 * windowSizeFactor) * getScaleFactor(octave): a keypoint 16 px away is outside at 1, inside at 2."""
    s = ps.point_scene(0.8, 0.5, [(16.0 / 1.2, 0.0, 0, 3)])               # the unit is getScaleFactor(1) = 1.2
    for wsf, want in ((1, matching.NO_CANDIDATES), (2, matching.MATCHED)):
        a = guided_args(s, [1], [0], wsf)
        g, r = host.guided_matching(*a), matching.guided_matching_ref(*a)
        for k in ("match", "status", "best", "second", "slot_point"):
            np.testing.assert_array_equal(getattr(g, k), r[k], err_msg=k)
        assert g.status[0] == want and r["radius"][0] == 15.0 * wsf
    with pytest.raises(ValueError):
        host.guided_matching(*guided_args(s, [1], [0], 1.5))


def frames(n_ref_points=3):
    """A reference keyframe whose first slots hold map points with descriptors, and a current keyframe with one
    keypoint per map point next to its projection; every current slot holds an earlier map point."""
    s = ps.point_scene(0.8, 0.5, [(2.0 * i - 2.0, 1.0, 0, 0) for i in range(n_ref_points)])
    inv = inv_sigma2_table(ps.N_SCALES, ps.FACTOR)
    ref = KeyFrame(0, ps.pose(), ps.KB8, n_ref_points + 1, inv, octaves=np.zeros(n_ref_points + 1, np.int32))
    cur = KeyFrame(1, s["Tcw"], ps.KB8, n_ref_points, inv, keypoints=s["uv2"], octaves=s["octave2"],
                   descriptors=np.stack([ms.first_bits(60 * i) for i in range(n_ref_points)]))
    for i in range(n_ref_points):
        mp = MapPoint(s["pos"][0], pid=100 + i)
        mp.descriptor = ms.first_bits(60 * i + 1)
        ref.map_points[i + 1] = mp                                         # slot 0 stays empty
    cur.map_points = [MapPoint(np.zeros(3), pid=900 + i) for i in range(n_ref_points)]
    return ref, cur


def test_guided_matching_clears_earlier_claims(host):
    ref, cur = frames()
    matches, report = matching.guided_matching(host, ref, cur, ps.GRID, 50, 1)
    np.testing.assert_array_equal(matches, [-1, 0, 1, 2])
    assert [mp.id for mp in cur.map_points] == [100, 101, 102] and report["n_matches"] == 3
    ref.map_points[2].descriptor = None
    with pytest.raises(ValueError, match="descriptor"):
        matching.guided_matching(host, ref, cur, ps.GRID, 50, 1)


def test_search_with_projection_sets_free_slots(host):
    ref, cur = frames()
    mps = [mp for mp in ref.map_points if mp is not None]
    with pytest.raises(ValueError, match="normal"):
        matching.search_with_projection(host, cur, ps.GRID, 50, mps)
    s = ps.point_scene(0.8, 0.5, [])
    for mp in mps:
        mp.normal, mp.min_distance, mp.max_distance = s["normal"][0], float(s["min_dist"][0]), float(s["max_dist"][0])
    keep = cur.map_points[1]
    cur.map_points = [None, keep, None]
    matches, report = matching.search_with_projection(host, cur, ps.GRID, 50, mps)
    np.testing.assert_array_equal(matches, [0, -1, 2])
    assert cur.map_points[1] is keep and [cur.map_points[0].id, cur.map_points[2].id] == [100, 102]
    assert report["n_matches"] == 2 and report["n_rejected"] == 1


def descriptor_case(bits, octaves=None, slots=None, n_slots=8):
    """One map point seen in len(bits) keyframes, observation i with its first bits[i] bits set, in slot slots[i]."""
    n = len(bits)
    slots = list(range(n)) if slots is None else slots
    d = ps.descriptor_scene(1, n, n_slots, seed=1)
    d["obs_start"], d["obs_kf"], d["obs_slot"] = np.array([0, n], np.int32), np.arange(n, dtype=np.int32), np.array(slots, np.int32)
    for k in range(n):
        d["kf_desc"][k * n_slots + slots[k]] = bits[k] if isinstance(bits[k], np.ndarray) else ms.first_bits(bits[k])
    if octaves is not None:
        d["kf_octave"][:] = np.asarray(octaves, np.int32).reshape(-1)
    return d


def run_descriptors(host, d):
    g, r = host.map_point_descriptors(*ps.descriptor_args(d)), matching.map_point_descriptors_ref(*ps.descriptor_args(d))
    for k in ("desc", "ref_obs", "status", "normal", "max_dist", "min_dist"):
        np.testing.assert_array_equal(getattr(g, k), r[k], err_msg=k)
    return g, r


def test_median_is_the_upper_one(host):
    g, r = run_descriptors(host, descriptor_case([0, 1, 12, 13]))          # medians 12 11 11 12; the lower ones tie at 1
    assert r["medians"][0] == [12, 11, 11, 12] and g.ref_obs[0] == 1
    g, r = run_descriptors(host, descriptor_case([0, 20, 21, 22, 50]))
    assert r["medians"][0] == [21, 2, 1, 2, 29] and g.ref_obs[0] == 2


def test_running_median_starts_at_255(host):
    zero = np.zeros(32, np.uint8)
    g, r = run_descriptors(host, descriptor_case([zero, ~zero]))           # both medians 256: not below 255
    assert r["medians"][0] == [256, 256] and g.ref_obs[0] == 0
    g, r = run_descriptors(host, descriptor_case([zero, ms.flip_bits(~zero, [9])]))
    assert r["medians"][0] == [255, 255] and g.ref_obs[0] == 0


def test_octave_is_read_at_the_ordinal(host):
    n_slots = 8
    octaves = np.zeros((3, n_slots), np.int32)
    octaves[1, 1], octaves[1, 5] = 4, 2                                    # observation 1 sits in slot 5 of keyframe 1
    d = descriptor_case([30, 10, 11], octaves, slots=[3, 5, 6], n_slots=n_slots)
    g, r = run_descriptors(host, d)
    assert g.ref_obs[0] == 1
    c = -(d["kf_Tcw"][1][:, :3].astype(np.float64).T @ d["kf_Tcw"][1][:, 3])
    dist = np.linalg.norm(d["pos"][0] - c)
    assert g.max_dist[0] == pytest.approx(dist * 1.2 ** 4, rel=1e-5)       # octave of keypoint 1, not of slot 5
    assert g.min_dist[0] == pytest.approx(dist * 1.2 ** 4 / 1.2 ** 7, rel=1e-5)
    d["kf_slot_start"] = np.array([0, 8, 9, 17], np.int32)                 # keyframe 1 with one slot: ordinal 1 is beyond it
    d["obs_slot"][1] = 0
    d["kf_desc"], d["kf_octave"] = d["kf_desc"][:17].copy(), d["kf_octave"][:17].copy()
    d["kf_desc"][8] = ms.first_bits(10)
    d["kf_desc"][9 + 6] = ms.first_bits(11)
    d["kf_desc"][3] = ms.first_bits(30)
    with pytest.raises(capi.DeftriError, match="ordinal"):
        host.map_point_descriptors(*ps.descriptor_args(d))
    with pytest.raises(ValueError, match="ordinal"):
        matching.map_point_descriptors_ref(*ps.descriptor_args(d))


def test_point_without_observations(host):
    d = ps.descriptor_scene(3, 4, 8, seed=2)
    a, b, c = d["obs_start"][1:]
    keep = np.r_[0:a, b:c]                                                 # point 1 loses its observations
    d["obs_start"] = np.array([0, a, a, a + c - b], np.int32)
    d["obs_kf"], d["obs_slot"] = d["obs_kf"][keep], d["obs_slot"][keep]
    g, r = run_descriptors(host, d)
    np.testing.assert_array_equal(g.status, [0, 1, 0])
    assert g.ref_obs[1] == -1 and not g.desc[1].any() and not g.normal[1].any()


def test_map_update_orientation_and_descriptor(host):
    ref, cur = frames()
    m = Map()
    ref.descriptors = np.stack([ms.first_bits(3 * i) for i in range(ref.n_slots)])
    for kf in (ref, cur):
        m.insert_keyframe(kf)
    cur.map_points = [None] * cur.n_slots
    for i, mp in enumerate(ref.map_points[1:]):
        mp.descriptor = None
        m.insert_map_point(mp)
        m.add_observation(ref.id, mp.id, i + 1)
        m.add_observation(cur.id, mp.id, i)
    lone = MapPoint(np.ones(3), pid=7)
    m.insert_map_point(lone)
    assert lone.descriptor is None and lone.normal is None and lone.min_distance is None and lone.max_distance is None
    with pytest.raises(ValueError):
        m.update_orientation_and_descriptor(host)
    status = m.update_orientation_and_descriptor(host, grid=ps.GRID)
    np.testing.assert_array_equal(status, [0, 0, 0, 1])
    assert lone.descriptor is None
    for mp in ref.map_points[1:]:
        # two observations: both medians are the mutual distance, the first in iteration order wins; with two
        # keyframes inserted as 0, 1 that order is the reverse insertion order, so keyframe 1 (cur) comes first
        order = capi.keyframe_order([ref.id, cur.id])
        first = {ref.id: ref, cur.id: cur}[order[0]]
        np.testing.assert_array_equal(mp.descriptor, first.descriptors[m.mp_obs[mp.id][first.id]])
        assert mp.normal.shape == (3,) and abs(np.linalg.norm(mp.normal) - 1) < 1e-6
        assert mp.max_distance >= mp.min_distance > 0


def test_abi(host):
    lib = capi.load()
    assert lib.deftri_abi_version() == 8
    assert lib.deftri_sizeof(20) == C.sizeof(_abi.ProjectionReport) == 64
    assert lib.deftri_sizeof(13) == -1 and lib.deftri_sizeof(19) == -1 and lib.deftri_sizeof(21) == -1
    for name in ("deftri_search_with_projection", "deftri_guided_matching", "deftri_map_point_descriptors"):
        assert name in capi.EXPORTED and hasattr(lib, name)


def test_argument_errors(host):
    s = ps.chain_scene()
    bad = dict(s, grid=dict(s["grid"], n_scales=1), octave2=np.zeros_like(s["octave2"]))
    with pytest.raises(capi.DeftriError, match="nScales < 2"):
        host.search_with_projection(*ps.args(bad))
    bad = dict(s, octave2=np.full_like(s["octave2"], 8))
    with pytest.raises(capi.DeftriError, match="octave 8"):
        host.search_with_projection(*ps.args(bad))
    with pytest.raises(capi.DeftriError, match="octave -1"):
        host.guided_matching(*guided_args(s, np.ones(len(s["pos"])), np.full(len(s["pos"]), -1), 1))
    bad = dict(s, grid=dict(s["grid"], cols=0))
    with pytest.raises(capi.DeftriError, match="nGridCols"):
        host.search_with_projection(*ps.args(bad))
    rc = capi.load().deftri_search_with_projection(host.h, None, None, None, 0, None, None, None, None, 0, None, None, None, None,
                                                   None, 50, None, None, None, None, None, None, None, None)
    assert rc == -1 and b"null" in capi.load().deftri_last_error(host.h)


def test_empty_inputs(host):
    s = ps.chain_scene()
    none = dict(s, pos=np.zeros((0, 3)), normal=np.zeros((0, 3)), min_dist=[], max_dist=[], desc=np.zeros((0, 32)))
    g = host.search_with_projection(*ps.args(none))
    assert len(g.match) == 0 and g.report["n_matches"] == 0
    np.testing.assert_array_equal(g.slot_point, s["slot_point"])
    none = dict(s, uv2=np.zeros((0, 2)), octave2=[], desc2=np.zeros((0, 32)), slot_point=[])
    g = host.search_with_projection(*ps.args(none))
    assert (g.match == -1).all() and g.report["n_points"] == 0
    d = ps.descriptor_scene(0, 2, 4)
    assert len(host.map_point_descriptors(*ps.descriptor_args(d)).status) == 0
