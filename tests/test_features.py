"""deftri_fast_extract on a host-only context against the numpy restatement of FAST::extract
(tests/features_ref.py): every output array and every count of the report equal, the pyramid levels byte for
byte and the candidates of every level through the debug entries, the argument errors with their messages,
and the mask reads against a windowed any().

Everything but the angle is integer arithmetic; the angle is a dozen float operations written in the same
order on both sides without contraction, so equality is exact there as well.

The scenes must exercise every branch of the restatement; test_scene_conditions asserts that on the
restatement's own outputs, so a scene that stops exercising one fails loudly."""
import numpy as np
import pytest

from deftri import _abi, capi, features, mapping, sim
from deftri.mapmodel import KeyFrame
from deftri.settings import Settings
import features_ref as fr

ARRAYS = ("uv", "octave", "angle", "response", "size")

# name: (rows, cols, seed, frame, n_scales, scale_factor, n_max_features, max_keys)
SCENES = {
    "160x120": (120, 160, 1, 0, 2, 1.2, 400, 300),
    "97x83_one_scale": (83, 97, 2, 0, 1, 1.2, 400, 300),                # odd sizes, one initial node, clipped last cells
    "240x180_realcolon_factor": (180, 240, 0, 0, 2, 1.66666666, 100, 300),
    "200x90_three_scales": (90, 200, 1, 0, 3, 1.2, 400, 300),           # nIni = 2; the last level is 139 x 62
    "border_mask": (120, 160, 1, 16, 2, 1.2, 400, 300),
    "max_keys_below_total": (180, 240, 1, 0, 2, 1.66666666, 400, 50),
}


def scene(name):
    rows, cols, seed, frame, n_scales, factor, n_max, max_keys = SCENES[name]
    image, border = fr.make_scene(rows, cols, seed, frame=frame)
    params = {"n_scales": n_scales, "scale_factor": factor, "n_max_features": n_max, "th_fast": 10, "min_th_fast": 4,
              "max_keys": max_keys}
    return image, border, params


_REF = {}


def reference(name):
    """The restatement's result for a scene, computed once and left unchanged."""
    if name not in _REF:
        image, border, p = scene(name)
        _REF[name] = fr.extract(image, p["n_scales"], p["scale_factor"], p["n_max_features"], p["th_fast"], p["min_th_fast"],
                                p["max_keys"], border)
    return _REF[name]


def assert_same_result(got, want_arrays, want_report):
    for k in ARRAYS:
        g, w = getattr(got, k), want_arrays[k]
        assert g.dtype == w.dtype and g.shape == w.shape, k
        np.testing.assert_array_equal(g, w, err_msg=k)
    for k, v in want_report.items():
        if not k.startswith("ms_") and k != "round_trips":
            assert got.report[k] == v, (k, got.report[k], v)


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


def test_struct_sizes():
    lib = capi.load()
    assert lib.deftri_sizeof(15) == capi.C.sizeof(_abi.FastParams)
    assert lib.deftri_sizeof(16) == capi.C.sizeof(_abi.FastReport)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_host_context_equals_restatement(host, name):
    image, border, p = scene(name)
    ref = reference(name)
    got = host.fast_extract(image, p, border)
    print(name, {k: v for k, v in got.report.items() if k.startswith("n_")})
    assert_same_result(got, ref, ref["report"])
    assert got.report["round_trips"] == 0 and len(got) == got.report["n_keys"] <= p["max_keys"]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_stages_equal_restatement(host, name):
    image, _border, p = scene(name)
    ref = reference(name)
    for level in range(p["n_scales"]):
        np.testing.assert_array_equal(host.debug_fast_pyramid(image, p, level), ref["levels"][level])
        xy, resp = host.debug_fast_candidates(image, p, level)
        want = np.array(ref["candidates"][level], np.int64).reshape(-1, 3)
        np.testing.assert_array_equal(xy, want[:, :2])
        np.testing.assert_array_equal(resp, want[:, 2].astype(np.float32))


def test_scene_conditions():
    """What the scene set must exercise, on the restatement alone."""
    refs = {n: reference(n) for n in SCENES}
    reports = [r["report"] for r in refs.values()]
    assert max(r["n_candidates"][0] for r in reports) >= 200
    assert any(sum(r["n_fallback_cells"]) > sum(r["n_empty_cells"]) for r in reports)      # a fallback that finds corners
    assert any(sum(r["n_empty_cells"]) > 0 for r in reports)
    assert any(r["masked"] for n, r in refs.items() if SCENES[n][3] == 0)                  # the reflection mask alone
    plain, framed = refs["160x120"], refs["border_mask"]                                   # the same image without / with a frame
    assert SCENES["160x120"][:3] == SCENES["border_mask"][:3]
    assert set(framed["masked"]) > set(plain["masked"])
    stats = [s for r in refs.values() for s in r["stats"]]
    assert any(s.get("sorted") and s.get("ties") for s in stats)
    assert any(s.get("single") for s in stats)
    assert sum(refs["max_keys_below_total"]["report"]["n_truncated"]) > 0
    angles = np.concatenate([r["angle"] for r in refs.values()])
    assert all(((angles >= 90 * q) & (angles < 90 * (q + 1))).any() for q in range(4))
    last = refs["200x90_three_scales"]["report"]
    assert (last["level_cols"][-1], last["level_rows"][-1]) == (139, 62)


def test_strided_image_and_no_keys(host):
    image, border, p = scene("160x120")
    wide = np.full((image.shape[0], image.shape[1] + 13), 255, np.uint8)
    wide[:, :image.shape[1]] = image
    view = wide[:, :image.shape[1]]
    assert view.strides[0] == image.shape[1] + 13
    assert_same_result(host.fast_extract(view, p), reference("160x120"), reference("160x120")["report"])
    none = host.fast_extract(image, dict(p, max_keys=0))
    assert len(none) == 0 and none.uv.shape == (0, 2) and sum(none.report["n_truncated"]) == sum(none.report["n_after_mask"]) > 0


ARG_ERRORS = [
    (dict(n_scales=0), None, "n_scales must be in \\[1, 16\\]"),
    (dict(n_scales=17), None, "n_scales must be in \\[1, 16\\]"),
    (dict(scale_factor=1.0), None, "scale_factor must be > 1"),
    (dict(th_fast=0), None, "1 <= min_th_fast <= th_fast <= 255"),
    (dict(th_fast=256), None, "1 <= min_th_fast <= th_fast <= 255"),
    (dict(min_th_fast=0), None, "1 <= min_th_fast <= th_fast <= 255"),
    (dict(min_th_fast=11), None, "1 <= min_th_fast <= th_fast <= 255"),
    (dict(max_keys=-1), None, "max_keys < 0"),
    (dict(n_max_features=-1), None, "n_max_features < 0"),
    (dict(), (61, 120), "level 0 \\(120 x 61\\) is below the 62 pixels"),
    (dict(), (120, 61), "level 0 \\(61 x 120\\) is below the 62 pixels"),
    (dict(n_scales=3), (88, 160), "level 2 \\(111 x 61\\) is below the 62 pixels"),
    (dict(n_scales=2, scale_factor=2.0), (120, 160), "level 1 \\(80 x 60\\) is below"),
    (dict(n_scales=2, scale_factor=2.0), (160, 200), "halves the level above it exactly"),
    (dict(), (200, 62), "round\\(width / height\\) = 0 nodes"),
]


@pytest.mark.parametrize("change,shape,message", ARG_ERRORS)
def test_argument_errors(host, change, shape, message):
    p = dict({"n_scales": 2, "scale_factor": 1.2, "n_max_features": 100, "th_fast": 10, "min_th_fast": 4, "max_keys": 50}, **change)
    image = np.zeros(shape or (120, 160), np.uint8)
    with pytest.raises(capi.DeftriError, match=message) as e:
        host.fast_extract(image, p)
    assert e.value.code == _abi.DEFTRI_E_ARG


def test_argument_errors_of_pointers_stride_and_mask(host):
    lib, C = host.lib, capi.C
    image = np.zeros((120, 160), np.uint8)
    p = _abi.FastParams(2, 1.2, 100, 10, 4, 50)
    uv = np.zeros((50, 2), np.float32); f = [np.zeros(50, np.float32) for _ in range(3)]; octave = np.zeros(50, np.int32)
    n = C.c_int32(0)
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    outs = (fp(uv), octave.ctypes.data_as(C.POINTER(C.c_int32)), fp(f[0]), fp(f[1]), fp(f[2]), C.byref(n), None)

    def message(rc):
        assert rc == _abi.DEFTRI_E_ARG
        return lib.deftri_last_error(host.h).decode()

    assert "null image, params or output" in message(lib.deftri_fast_extract(host.h, None, 120, 160, 160, None, 0, 0, 0, C.byref(p), *outs))
    assert "null image, params or output" in message(lib.deftri_fast_extract(host.h, u8(image), 120, 160, 160, None, 0, 0, 0, None, *outs))
    assert "null image, params or output" in message(
        lib.deftri_fast_extract(host.h, u8(image), 120, 160, 160, None, 0, 0, 0, C.byref(p), None, *outs[1:]))
    assert "stride < cols" in message(lib.deftri_fast_extract(host.h, u8(image), 120, 160, 159, None, 0, 0, 0, C.byref(p), *outs))
    with pytest.raises(capi.DeftriError, match="the border mask is 159 x 120, the image 160 x 120") as e:
        host.fast_extract(image, p, np.zeros((120, 159), np.uint8))
    assert e.value.code == _abi.DEFTRI_E_ARG
    with pytest.raises(capi.DeftriError, match="level outside"):
        host.debug_fast_pyramid(image, p, 2)
    with pytest.raises(ValueError, match="8-bit single-channel"):
        host.fast_extract(image.astype(np.float32), p)


def test_mask_reads_equal_a_windowed_any(host):
    """The library's mask method (an integral image of the base mask) against the dilation's definition, on a
    300 x 260 mask, 1000 random positions per level up to level 5 (side 219)."""
    rng = np.random.default_rng(11)
    image, _ = fr.make_scene(260, 300, 7, n_blobs=2)
    border = np.zeros_like(image)
    border[:, :3] = 1; border[-2:, :] = 200; border[40:43, 250:255] = 9
    base = fr.base_mask(image, border)
    assert base.any() and not base.all()
    assert [fr.mask_side(l) for l in range(6)] == [13, 19, 33, 59, 113, 219]
    seen = set()
    for level in range(6):
        xy = np.stack([rng.integers(0, 300, 1000), rng.integers(0, 260, 1000)], 1).astype(np.int32)
        xy[:4] = [[0, 0], [299, 259], [0, 259], [299, 0]]
        got = host.debug_fast_mask(image, level, xy, border)
        want = np.array([fr.mask_read(base, level, x, y) for x, y in xy])
        np.testing.assert_array_equal(got, want)
        seen |= set(want.tolist())
        plain = host.debug_fast_mask(image, level, xy)
        np.testing.assert_array_equal(plain, np.array([fr.mask_read(fr.base_mask(image), level, x, y) for x, y in xy]))
    assert seen == {True, False}


def test_settings_and_keyframe_helpers(host):
    text = ("FeatureExtractor.nScales: 2\nFeatureExtractor.fScaleFactor: 1.2\nFeatureExtractor.nFeatures: 150\n"
            "FeatureExtractor.imageBoderMask: \"masks/border.png\"\n")
    s = Settings(text=text)
    assert s.border_mask_path == "masks/border.png" and Settings(text="").border_mask_path == ""
    assert features.fast_params(s) == {"n_scales": 2, "scale_factor": 1.2, "n_max_features": 300, "th_fast": 10, "min_th_fast": 4,
                                       "max_keys": 150}
    image, border, _ = scene("border_mask")
    with pytest.raises(ValueError, match="decode it and pass border_mask"):
        features.extract(host, image, s)
    res = features.extract(host, image, s, border)
    ref = fr.extract(image, 2, 1.2, 300, 10, 4, 150, border)
    assert_same_result(res, ref, ref["report"])
    kf = KeyFrame(0, None, np.zeros(8), 150, sim.inv_sigma2_table(2, 1.2))
    assert kf.angles is None
    n = mapping.set_keypoints_from_features(kf, res)
    assert n == len(res) > 0
    np.testing.assert_array_equal(kf.keypoints[:n], res.uv)
    np.testing.assert_array_equal(kf.octaves[:n], res.octave)
    np.testing.assert_array_equal(kf.angles[:n], res.angle)
    assert not kf.keypoints[n:].any() and not kf.angles[n:].any()
    with pytest.raises(ValueError, match="slots"):
        mapping.set_keypoints_from_features(KeyFrame(1, None, np.zeros(8), n - 1, sim.inv_sigma2_table(2, 1.2)), res)
