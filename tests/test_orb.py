"""deftri_orb_describe on a host-only context against the numpy restatement of ORB::describe
(tests/orb_ref.py): every pyramid level with its border byte for byte through the debug entry, descriptors and
status equal, the integer blur kernel, the saturation, the argument errors with their messages, and the
Python surface above it (features.describe, mapping.extract_features, set_keypoints_from_features).

Everything is integer arithmetic but the keypoint's centre and the rotated sample offsets: a handful of float
operations written in the same order on both sides without contraction, with cos and sin from the same libm,
so equality is exact.  The sampling patterns are seeded synthetic ones; the reference's table is in no file
here.

The scenes must exercise every branch of the restatement; test_scene_conditions asserts that on the
restatement's own numbers, so a scene that stops exercising one fails loudly."""
import numpy as np
import pytest

from deftri import _abi, capi, features, mapping, sim
from deftri.mapmodel import KeyFrame
from deftri.settings import Settings
import features_ref as fr
import orb_ref as ref

# name: (rows, cols, seed, n_scales, scale_factor)
SCENES = {
    "160x120": (120, 160, 1, 2, 1.2),
    "97x83_one_scale": (83, 97, 2, 1, 1.2),                 # odd sizes, one level
    "200x90_three_scales": (90, 200, 1, 3, 1.2),
    "240x180_realcolon_factor": (180, 240, 0, 2, 1.66666666),
}
LARGEST = "240x180_realcolon_factor"
ANGLES = (0.0, 30.0, 45.0, 90.0, 180.0, 270.0, 359.99)
PATTERN = ref.synthetic_pattern(7)

_CASES, _REF = {}, {}


def scene(name):
    """(image, orb params, uv, octave, angle, number of fr.extract keypoints): the keypoints of fr.extract for the
    scene, then hand-placed ones at every octave, one per angle of ANGLES, at and next to the level's edges (with
    PATTERN's 18-pixel reach they read the border and stay inside it) and at its centre."""
    if name not in _CASES:
        rows, cols, seed, n_scales, factor = SCENES[name]
        image, _ = fr.make_scene(rows, cols, seed)
        keys = fr.extract(image, n_scales, factor, 400, 10, 4, 300)
        scale, inv = ref.scale_tables(n_scales, factor)
        uv, octave, angle = [keys["uv"]], [keys["octave"]], [keys["angle"]]
        for l in range(n_scales):
            lr, lc = fr.cv_round(np.float32(rows) * inv[l]), fr.cv_round(np.float32(cols) * inv[l])
            spots = [(0, 0), (lc - 1, lr - 1), (1, lr - 2), (lc - 2, 1), (lc // 2, lr // 2), (0, lr // 2), (lc // 3, lr - 1)]
            for (x, y), ang in zip(spots, ANGLES):
                uv.append(np.array([[np.float32(x) * scale[l], np.float32(y) * scale[l]]], np.float32))
                octave.append(np.array([l], np.int32))
                angle.append(np.array([ang], np.float32))
        _CASES[name] = (image, {"n_scales": n_scales, "scale_factor": factor}, np.concatenate(uv), np.concatenate(octave),
                        np.concatenate(angle), len(keys["octave"]))
    return _CASES[name]


def reference(name):
    """The restatement's result for a scene, computed once and left unchanged."""
    if name not in _REF:
        image, p, uv, octave, angle, _ = scene(name)
        _REF[name] = ref.describe(image, p["n_scales"], p["scale_factor"], uv, octave, angle, PATTERN)
    return _REF[name]


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    ctx.orb_set_pattern(PATTERN)
    yield ctx
    ctx.close()


def test_struct_sizes():
    lib = capi.load()
    assert lib.deftri_sizeof(17) == capi.C.sizeof(_abi.OrbParams) == 8
    assert lib.deftri_sizeof(18) == capi.C.sizeof(_abi.OrbReport)
    assert lib.deftri_sizeof(13) == -1 and lib.deftri_sizeof(19) == -1


def test_blur_kernel():
    k = np.zeros(7, np.int32)
    assert capi.load().deftri_debug_orb_blur_kernel(k.ctypes.data_as(capi.C.POINTER(capi.C.c_int32))) == 0
    assert k.tolist() == [18, 34, 49, 55, 49, 34, 18] == ref.blur_kernel().tolist()
    assert k.sum() == 257


@pytest.mark.parametrize("name", sorted(SCENES))
def test_pyramid_equals_restatement(host, name):
    image, p, *_ = scene(name)
    want = reference(name)["levels"]
    for level in range(p["n_scales"]):
        got = host.debug_orb_pyramid(image, p, level)
        assert got.shape == want[level].shape
        np.testing.assert_array_equal(got, want[level], err_msg=f"level {level}")
    with pytest.raises(capi.DeftriError, match="level outside"):
        host.debug_orb_pyramid(image, p, p["n_scales"])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_host_context_equals_restatement(host, name):
    image, p, uv, octave, angle, _ = scene(name)
    want = reference(name)
    got = host.orb_describe(image, p, uv, octave, angle)
    assert got.desc.dtype == np.uint8 and got.desc.shape == (len(octave), 32)
    np.testing.assert_array_equal(got.status, want["status"])
    np.testing.assert_array_equal(got.desc, want["desc"])
    rep = got.report
    print(name, {k: v for k, v in rep.items() if not k.startswith("ms_")})
    assert rep["n_keys"] == len(octave) and rep["n_outside"] == 0 and rep["round_trips"] == 0 and rep["n_levels"] == p["n_scales"]
    assert list(zip(rep["level_rows"], rep["level_cols"])) == [a.shape for a in want["plains"]]


def test_scene_conditions():
    """What the scene set must exercise, on the restatement alone."""
    refs = {n: reference(n) for n in SCENES}
    # a sample offset that is an exact k + 0.5 before rounding: the rounding rule decides it
    ties = sum(int((np.abs(raw - np.floor(raw)) == 0.5).sum()) for r in refs.values() for pair in r["raw"] for raw in pair)
    assert ties > 0
    border_reads = differs = cascade = 0
    for name, r in refs.items():
        n_fast = scene(name)[5]
        # only described keypoints, and every fr.extract keypoint among them
        assert not r["status"].any() and n_fast > 0
        for l, (level, plain) in enumerate(zip(r["levels"], r["plains"])):
            lr, lc = plain.shape
            # a border pixel that a blur of the bordered image would have changed
            full = ref.blur_u8(ref.add_border(plain))
            edge = np.ones(level.shape, bool)
            edge[ref.BORDER:-ref.BORDER, ref.BORDER:-ref.BORDER] = False
            differs += int((full[edge] != level[edge]).sum())
            if l:                                              # the cascade: the level above was blurred before the resize
                cascade += int((plain != fr.resize_linear_u8(r["plains"][l - 1], lr, lc)).sum())
        for k, (rows, cols) in enumerate(zip(r["rows"], r["cols"])):
            lr, lc = r["plains"][int(scene(name)[3][k])].shape
            border_reads += int(((rows < 0) | (rows >= lr) | (cols < 0) | (cols >= lc)).any())
    assert border_reads > 0 and differs > 0 and cascade > 0
    desc = refs[LARGEST]["desc"]
    assert len(np.unique(desc, axis=0)) > 1
    bits = np.unpackbits(desc, axis=1)
    assert bits.any(0).all() and not bits.all(0).any()         # both values in every bit position's column


def test_saturation_and_smallest_level(host):
    """The kernel sums to 257: a constant 255 area needs the saturation.  40 x 40 at 1.9 also has a 21 x 21 level,
    next to the 20-pixel limit."""
    image = np.full((40, 40), 255, np.uint8)
    p = {"n_scales": 2, "scale_factor": 1.9}
    for level, side in ((0, 40), (1, 21)):
        got = host.debug_orb_pyramid(image, p, level)
        assert got.shape == (side + 38, side + 38) and (got == 255).all()
    assert (ref.blur_u8(image) == 255).all() and int(ref.blur_kernel().sum()) ** 2 * 255 + 32768 >= 256 << 16
    textured, _ = fr.make_scene(40, 40, 4)
    want = ref.pyramid(textured, ref.scale_tables(2, 1.9)[1])[0]
    assert want[1].shape == (59, 59)
    for level in range(2):
        np.testing.assert_array_equal(host.debug_orb_pyramid(textured, p, level), want[level])
    smallest = {"n_scales": 2, "scale_factor": 2.0000002}     # 40 -> 20 would halve exactly; 41 -> 20 does not
    textured41, _ = fr.make_scene(41, 41, 4)
    want = ref.pyramid(textured41, ref.scale_tables(2, 2.0000002)[1])[0]
    assert want[1].shape == (58, 58)
    np.testing.assert_array_equal(host.debug_orb_pyramid(textured41, smallest, 1), want[1])


def corner_case(name):
    """A lim = 15 pattern whose first four points are the patch's corners, and keypoints at 45 degrees at the four
    corners of each level and up to 3 pixels inside: the corner points reach 21 pixels there.  Then keypoints with
    a non-finite coordinate or angle."""
    image, p, uv, octave, angle, n_fast = scene(name)
    rows, cols = image.shape
    pattern = ref.synthetic_pattern(11, 15)
    pattern[:4] = [[15, 15], [-15, -15], [15, -15], [-15, 15]]
    scale, inv = ref.scale_tables(p["n_scales"], p["scale_factor"])
    uv, octave, angle = [uv[:n_fast]], [octave[:n_fast]], [angle[:n_fast]]
    corners = []
    for l in range(p["n_scales"]):
        lr, lc = fr.cv_round(np.float32(rows) * inv[l]), fr.cv_round(np.float32(cols) * inv[l])
        for inset in range(4):
            for x, y in ((inset, inset), (lc - 1 - inset, inset), (inset, lr - 1 - inset), (lc - 1 - inset, lr - 1 - inset)):
                corners.append(inset)
                uv.append(np.array([[np.float32(x) * scale[l], np.float32(y) * scale[l]]], np.float32))
                octave.append(np.array([l], np.int32))
                angle.append(np.array([45.0], np.float32))
    odd = [((np.nan, 10.0), 0.0), ((10.0, np.inf), 0.0), ((50.0, 50.0), np.nan), ((50.0, 50.0), np.inf), ((-1e30, 3e38), 10.0)]
    for xy, ang in odd:
        uv.append(np.array([xy], np.float32)); octave.append(np.array([0], np.int32)); angle.append(np.array([ang], np.float32))
    return image, p, pattern, np.concatenate(uv), np.concatenate(octave), np.concatenate(angle), n_fast, np.array(corners), len(odd)


@pytest.mark.parametrize("name", ["160x120", "200x90_three_scales"])
def test_status_of_keypoints_that_read_outside(name):
    image, p, pattern, uv, octave, angle, n_fast, corners, n_odd = corner_case(name)
    want = ref.describe(image, p["n_scales"], p["scale_factor"], uv, octave, angle, pattern)
    st = want["status"]
    # on the restatement: every fr.extract keypoint is described; the corners and one pixel inside are not
    assert not st[:n_fast].any()
    hand = st[n_fast:len(st) - n_odd]
    assert hand[corners <= 1].all() and not hand[corners == 3].all() and st[len(st) - n_odd:].all()
    with capi.Context(-1) as ctx:
        ctx.orb_set_pattern(pattern)
        got = ctx.orb_describe(image, p, uv, octave, angle)
    np.testing.assert_array_equal(got.status, st)
    np.testing.assert_array_equal(got.desc, want["desc"])
    assert not got.desc[st == 1].any() and got.report["n_outside"] == int(st.sum()) > 0


def test_pattern_replacement_and_shapes(host):
    image, p, uv, octave, angle, _ = scene("97x83_one_scale")
    other = ref.synthetic_pattern(8)
    with capi.Context(-1) as ctx:
        ctx.orb_set_pattern(other.reshape(256, 4))
        first = ctx.orb_describe(image, p, uv, octave, angle)
        np.testing.assert_array_equal(first.desc, ref.describe(image, 1, 1.2, uv, octave, angle, other)["desc"])
        ctx.orb_set_pattern(PATTERN)
        second = ctx.orb_describe(image, p, uv, octave, angle)
    np.testing.assert_array_equal(second.desc, reference("97x83_one_scale")["desc"])
    assert (first.desc != second.desc).any()
    for bad in (PATTERN[:500], PATTERN.astype(np.float32), PATTERN.reshape(1024)):
        with pytest.raises(ValueError, match="shape \\(512, 2\\) or \\(256, 4\\)"):
            host.orb_set_pattern(bad)


def test_no_keys_and_strided_image(host):
    image, p, uv, octave, angle, _ = scene("160x120")
    none = host.orb_describe(image, p, np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert none.desc.shape == (0, 32) and none.status.shape == (0,) and none.report["n_keys"] == 0
    assert none.report["level_cols"] == [160, 133]
    lib, C = host.lib, capi.C
    prm = _abi.OrbParams(2, 1.2)
    assert lib.deftri_orb_describe(host.h, image.ctypes.data_as(C.POINTER(C.c_uint8)), 120, 160, 160, C.byref(prm), 0, None, None, None,
                                   None, None, None) == 0
    wide = np.full((image.shape[0], image.shape[1] + 13), 255, np.uint8)
    wide[:, :image.shape[1]] = image
    got = host.orb_describe(wide[:, :image.shape[1]], p, uv, octave, angle)
    np.testing.assert_array_equal(got.desc, reference("160x120")["desc"])


ARG_ERRORS = [
    (dict(n_scales=0), None, None, "n_scales must be in \\[1, 16\\]"),
    (dict(n_scales=17), None, None, "n_scales must be in \\[1, 16\\]"),
    (dict(scale_factor=1.0), None, None, "scale_factor must be > 1"),
    (dict(), None, 2, "keypoint 0: octave 2 outside \\[0, n_scales\\)"),
    (dict(), None, -1, "keypoint 0: octave -1 outside \\[0, n_scales\\)"),
    (dict(), (19, 40), None, "level 0 \\(40 x 19\\) is below the 20 pixels"),
    (dict(), (40, 19), None, "level 0 \\(19 x 40\\) is below the 20 pixels"),
    (dict(n_scales=3), (28, 60), None, "level 2 \\(42 x 19\\) is below the 20 pixels"),
    (dict(scale_factor=2.0), (40, 60), None, "halves the level above it exactly"),
]


@pytest.mark.parametrize("change,shape,octave,message", ARG_ERRORS)
def test_argument_errors(host, change, shape, octave, message):
    p = dict({"n_scales": 2, "scale_factor": 1.2}, **change)
    image = np.zeros(shape or (120, 160), np.uint8)
    with pytest.raises(capi.DeftriError, match=message) as e:
        host.orb_describe(image, p, np.array([[30.0, 30.0]], np.float32), [octave or 0], [0.0])
    assert e.value.code == _abi.DEFTRI_E_ARG


def test_argument_errors_of_pointers_stride_pattern_and_n(host):
    lib, C = host.lib, capi.C
    image = np.zeros((120, 160), np.uint8)
    p = _abi.OrbParams(2, 1.2)
    uv = np.zeros((4, 2), np.float32); octave = np.zeros(4, np.int32); angle = np.zeros(4, np.float32)
    desc = np.zeros((4, 32), np.uint8); status = np.zeros(4, np.uint8)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    full = [host.h, u8(image), 120, 160, 160, C.byref(p), 4, fp(uv), ip(octave), fp(angle), u8(desc), u8(status), None]

    def message(ctx, rc):
        assert rc == _abi.DEFTRI_E_ARG
        return lib.deftri_last_error(ctx.h).decode()

    for at in (1, 5, 7, 8, 9, 10, 11):                          # image, params, uv, octave, angle, desc, status
        args = list(full)
        args[at] = None
        assert "null image, params, keypoints or output" in message(host, lib.deftri_orb_describe(*args))
    args = list(full); args[4] = 159
    assert "stride < cols" in message(host, lib.deftri_orb_describe(*args))
    args = list(full); args[6] = -1
    assert "n < 0" in message(host, lib.deftri_orb_describe(*args))
    assert "null pattern" in message(host, lib.deftri_orb_set_pattern(host.h, None))
    with capi.Context(-1) as fresh:                            # describe before set_pattern
        with pytest.raises(capi.DeftriError, match="no pattern set: pass the 512 sampling points to deftri_orb_set_pattern") as e:
            fresh.orb_describe(image, p, uv, octave, angle)
        assert e.value.code == _abi.DEFTRI_E_ARG
        fresh.debug_orb_pyramid(image, p, 1)                   # the pyramid needs none
        for value, where in ((16, "point 3 x 16"), (-16, "point 3 x -16")):
            bad = PATTERN.copy()
            bad[3, 0] = value
            with pytest.raises(capi.DeftriError, match=where + " outside \\[-15, 15\\]") as e:
                fresh.orb_set_pattern(bad)
            assert e.value.code == _abi.DEFTRI_E_ARG
        bad = PATTERN.copy()
        bad[511, 1] = 16
        with pytest.raises(capi.DeftriError, match="point 511 y 16 outside"):
            fresh.orb_set_pattern(bad)
        edge = PATTERN.copy()
        edge[0] = [15, -15]
        fresh.orb_set_pattern(edge)                            # the limits themselves are inside
    with pytest.raises(ValueError, match="8-bit single-channel"):
        host.orb_describe(image.astype(np.float32), p, uv, octave, angle)


def test_settings_extract_features_and_keyframe_helpers(host):
    text = "FeatureExtractor.nScales: 2\nFeatureExtractor.fScaleFactor: 1.2\nFeatureExtractor.nFeatures: 150\n"
    s = Settings(text=text)
    assert features.orb_params(s) == {"n_scales": 2, "scale_factor": 1.2}
    image = scene("160x120")[0]
    with pytest.raises(ValueError, match="bit_pattern_31_ from your copy of the reference"):
        features.describe(host, image, features.extract(host, image, s), s, None)
    with capi.Context(-1) as ctx:
        keys, described = mapping.extract_features(ctx, image, s, PATTERN.reshape(256, 4))
        want_keys = features.extract(ctx, image, s)
        want = features.describe(ctx, image, (want_keys.uv, want_keys.octave, want_keys.angle), s, PATTERN)
    for k in ("uv", "octave", "angle", "response", "size"):
        np.testing.assert_array_equal(getattr(keys, k), getattr(want_keys, k))
    np.testing.assert_array_equal(described.desc, want.desc)
    np.testing.assert_array_equal(described.status, want.status)
    n = len(keys)
    assert n > 0 and len(described) == n and not described.status.any()
    np.testing.assert_array_equal(described.desc, ref.describe(image, 2, 1.2, keys.uv, keys.octave, keys.angle, PATTERN)["desc"])
    # without the new argument the descriptors stay as they were
    kf = KeyFrame(0, None, np.zeros(8), 150, sim.inv_sigma2_table(2, 1.2))
    assert mapping.set_keypoints_from_features(kf, keys) == n and kf.descriptors is None
    mine = np.arange(150 * 32, dtype=np.uint8).reshape(150, 32)
    kf2 = KeyFrame(1, None, np.zeros(8), 150, sim.inv_sigma2_table(2, 1.2), descriptors=mine.copy())
    mapping.set_keypoints_from_features(kf2, keys)
    np.testing.assert_array_equal(kf2.descriptors, mine)
    # with it they are ORB::describe's, zeros behind the keypoints
    assert mapping.set_keypoints_from_features(kf2, keys, described) == n
    assert kf2.descriptors.shape == (150, 32) and kf2.descriptors.dtype == np.uint8
    np.testing.assert_array_equal(kf2.descriptors[:n], described.desc)
    assert not kf2.descriptors[n:].any()
    np.testing.assert_array_equal(kf2.keypoints[:n], keys.uv)
    with pytest.raises(ValueError, match="descriptors for"):
        mapping.set_keypoints_from_features(kf2, keys, capi.OrbResult(described.desc[:-1], described.status[:-1], {}))
