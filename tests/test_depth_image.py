"""Real-image input on a host-only context: KeyFrame::getDepthMeasure from a keyframe's depth image
(deftri_set_depth_images / deftri_depth_measure) against the float32 numpy restatement
(tests/depth_image_ref.py) bit for bit, the per-pixel status, and the graph builds that read their
depth measurements from the images."""
import copy
import ctypes as C

import numpy as np
import pytest

from deftri import _abi, capi, sim
import depth_image_ref as ref

SIGMA = np.float32(0.003)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _image(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return (10 + 5 * rng.random((rows, cols))).astype(np.float32)


def _edge_pixels(rows, cols):
    """(uv, expected status): integer coordinates, the next-row spill at x = cols-1 on a non-last row,
    y in the last row, x >= cols / y >= rows, negative and NaN."""
    px = [((0, 0), 0), ((1, 1), 0), ((cols - 2, rows - 2), 0), ((2.5, 1.25), 0),
          ((cols - 1, 0), 0), ((cols - 1 + 0.5, 1.5), 0), ((cols - 0.25, rows - 3), 0),        # spill: defined memory
          ((cols - 1, rows - 2), 2),                                                             # its last index = rows*cols
          ((0, rows - 1), 2), ((1.5, rows - 1 + 0.5), 2), ((cols - 1, rows - 1), 2),             # y in the last row
          ((cols, 0), 1), ((cols + 3.5, 1), 1), ((0, rows), 1), ((1, rows + 2.25), 1), ((np.inf, 1), 1),
          ((np.nan, rows), 1),                                                                   # y >= rows is tested first
          ((-0.5, 1), 2), ((1, -1), 2), ((-3, -3), 2), ((np.nan, 1), 2), ((1, np.nan), 2), ((-np.inf, 1), 2)]
    return np.array([p for p, _ in px], np.float32), np.array([s for _, s in px], np.uint8)


@pytest.mark.parametrize("rows,cols", [(5, 7), (33, 17)])
def test_sampler_equals_the_restatement_bit_for_bit(rows, cols):
    img = _image(rows, cols, rows)
    rng = np.random.default_rng(cols)
    uv = np.column_stack([rng.uniform(-1, cols + 1, 1000), rng.uniform(-1, rows + 1, 1000)]).astype(np.float32)
    edge, want = _edge_pixels(rows, cols)
    uv = np.concatenate([uv, edge])
    with capi.Context(-1) as ctx:
        ctx.set_depth_images([(7, img, 1.75, [1, 1, 0, 0])])
        for scaled in (True, False):
            d, st = ctx.depth_measure(7, uv, scaled)
            d_ref, st_ref = ref.sample(img, uv, 1.75, scaled)
            assert np.array_equal(st, st_ref)
            assert np.array_equal(st[-len(edge):], want)
            ok = st == 0
            assert ok.sum() > 300 and (st == 1).sum() > 20 and (st == 2).sum() > 20
            assert np.array_equal(_bits(d[ok]), _bits(d_ref[ok]))
            assert np.isnan(d[~ok]).all()
        # the spill reads the next row's first pixel
        d, st = ctx.depth_measure(7, [[cols - 1, 0]], True)
        assert st[0] == 0 and d[0] == float(img[0, cols - 1]) / 100
        d, st = ctx.depth_measure(7, [[cols - 0.5, 0]], True)
        assert st[0] == 0 and d[0] == float(np.float32(np.float32(img[0, cols - 1] * np.float32(0.5)) +
                                                       np.float32(img[1, 0] * np.float32(0.5)))) / 100
        # n = 0
        d, st = ctx.depth_measure(7, np.zeros((0, 2), np.float32))
        assert len(d) == 0 and len(st) == 0
        # no image for that keyframe
        with pytest.raises(capi.DeftriError) as e:
            ctx.depth_measure(8, uv)
        assert e.value.code == _abi.DEFTRI_E_ARG
        assert ctx.depth_image_stats() == (1, 0)


def _maps():
    m2, _ = sim.simulate_two_view(n=300, seed=3)
    m3, _ = sim.simulate_multi_view(n=200, k=3, seed=4)
    return [ref.synthetic_images(m2, (560, 640), seed=7), ref.synthetic_images(m3, (300, 330), seed=8)]


@pytest.fixture(scope="module")
def image_maps():
    return _maps()


def _same_but_dep_meas(p, q):
    for f in ("points", "tg", "scales", "cam_kb8", "cam_pose", "rep_point", "rep_cam", "rep_obs", "rep_info", "dep_point",
              "dep_scale", "dep_cam", "dep_info", "arap_pts", "arap_pair", "arap_rot", "arap_w", "rot", "pair_area",
              "pair_info", "order_xy"):
        a, b = getattr(p, f), getattr(q, f)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f
    assert np.array_equal(p.point_ids, q.point_ids)


def _without_images(m):
    t = copy.deepcopy(m)
    for kf in t.keyframes.values():
        kf.set_depth_image(None)
    return t


@pytest.mark.parametrize("which", [0, 1])
def test_graph_reads_the_images(image_maps, which):
    m = image_maps[which]
    # the lookups are near the simulated depths (the images are a plausible stand-in)
    for kf in m.keyframes.values():
        d, st = ref.keyframe_depths(kf, False)
        assert (st == 0).all() and np.abs(d - kf.depth).max() < 0.5 * kf.depth.max()
    with capi.Context(-1) as ctx, capi.Context(-1) as plain:
        p_img = ctx.build_graph(m, 1.0, 2e5, SIGMA)
        assert ctx.depth_image_stats() == (len(m.keyframes), len(m.keyframes))
        p_idx = plain.build_graph(_without_images(m), 1.0, 2e5, SIGMA)
        assert plain.depth_image_stats() == (0, 0)               # maps without images: today's path
        tags = plain.build_graph(ref.tagged(m), 1.0, 2e5, SIGMA).dep_meas
        _same_but_dep_meas(p_img, p_idx)
        assert len(tags) == len(p_img.dep_meas) > 0
        assert np.array_equal(_bits(p_img.dep_meas), _bits(ref.dep_meas_from_tags(m, tags)))
        assert not np.array_equal(p_img.dep_meas, p_idx.dep_meas)
        # a keyframe with an image needs no per-index depths
        bare = copy.deepcopy(m)
        for kf in bare.keyframes.values():
            kf.depth = None
        assert np.array_equal(_bits(ctx.build_graph(bare, 1.0, 2e5, SIGMA).dep_meas), _bits(p_img.dep_meas))
        assert ctx.depth_image_stats() == (len(m.keyframes), len(m.keyframes))     # same set, same keypoints: cached
        # a mixed map: the first keyframe without an image
        mixed = copy.deepcopy(m)
        first = next(iter(mixed.keyframes.values()))
        first.set_depth_image(None)
        p_mix = ctx.build_graph(mixed, 1.0, 2e5, SIGMA)
        _same_but_dep_meas(p_mix, p_idx)
        want = ref.dep_meas_from_tags(mixed, tags)
        assert np.array_equal(_bits(p_mix.dep_meas), _bits(want))
        from_index = (tags.astype(np.int64) // 4096) == first.id
        assert from_index.any() and np.array_equal(p_mix.dep_meas[from_index], p_idx.dep_meas[from_index])
        # n = 0 restores the per-index descriptor
        ctx.set_depth_images([])
        p_back = ctx.build_graph(_without_images(m), 1.0, 2e5, SIGMA)
        _same_but_dep_meas(p_back, p_idx)
        assert np.array_equal(_bits(p_back.dep_meas), _bits(p_idx.dep_meas))


def test_observation_outside_the_image(image_maps):
    m = copy.deepcopy(image_maps[0])
    kf = m.keyframes[0]
    rows, cols = kf.depth_image.shape
    with capi.Context(-1) as ctx:
        good = ctx.build_graph(m, 1.0, 2e5, SIGMA)
        # an observation no slot uses: fine, whatever its pixel
        mp = kf.map_points[5]
        idx = m.is_map_point_in_keyframe(mp.id, kf.id)
        used_uv = kf.keypoints[idx].copy()
        m.remove_observation(kf.id, mp.id)
        kf.keypoints[idx] = [cols + 10, 3]
        p = ctx.build_graph(m, 1.0, 2e5, SIGMA)
        assert len(p.dep_meas) == len(good.dep_meas) - 2
        # a used one: DEFTRI_E_ARG naming the keyframe, the observation and the pixel; the map is untouched
        m.add_observation(kf.id, mp.id, idx)
        before = [q.position.copy() for q in m.map_points.values()]
        for uv, word in (([cols + 10, 3], "out of range"), ([3.5, rows - 0.5], "outside")):
            kf.keypoints[idx] = uv
            with pytest.raises(capi.DeftriError) as e:
                ctx.build_graph(m, 1.0, 2e5, SIGMA)
            assert e.value.code == _abi.DEFTRI_E_ARG
            msg = str(e.value)
            assert f"keyframe {kf.id}" in msg and f"observation {idx}" in msg and word in msg
            assert f"({uv[0]:g}, {uv[1]:g})" in msg
        assert all(np.array_equal(a, q.position) for a, q in zip(before, m.map_points.values()))
        # and the context still builds the repaired map
        kf.keypoints[idx] = used_uv
        again = ctx.build_graph(m, 1.0, 2e5, SIGMA)
        assert np.array_equal(_bits(again.dep_meas), _bits(good.dep_meas))


def test_clone_shares_the_image_and_struct_sizes(image_maps):
    m = image_maps[1]
    for c in (m.clone(), copy.deepcopy(m)):
        for kid, kf in m.keyframes.items():
            assert c.keyframes[kid].depth_image is kf.depth_image
            assert c.keyframes[kid].image_depth_scale == kf.image_depth_scale
            assert c.keyframes[kid].keypoints is not kf.keypoints
    lib = capi.load()
    assert lib.deftri_sizeof(11) == C.sizeof(_abi.DepthImageC)
    assert lib.deftri_sizeof(12) == C.sizeof(_abi.RealAbsErrorsC)
    assert lib.deftri_sizeof(13) == -1
    # a clone on the same context re-sends nothing and samples nothing anew
    with capi.Context(-1) as ctx:
        a = ctx.build_graph(m, 1.0, 2e5, SIGMA)
        b = ctx.build_graph(m.clone(), 1.0, 2e5, SIGMA)
        assert ctx.depth_image_stats() == (3, 3)
        # (the clone iterates its keyframes in another order: the same measurements, other rows)
        assert np.array_equal(np.sort(a.dep_meas), np.sort(b.dep_meas))
        # other arrays with the same content (a map a worker process unpickled): not re-sent either
        import pickle
        ctx.build_graph(pickle.loads(pickle.dumps(m)), 1.0, 2e5, SIGMA)
        assert ctx.depth_image_stats() == (3, 3)
