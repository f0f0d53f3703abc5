"""deftri_orb_describe on the device (k_resize, k_orb_level, k_orb_describe) against the library's sequential
host loops on a host-only context: every pyramid level with its border through the debug entry, descriptors,
status and the report's counts bit for bit (both sides run the same integer arithmetic and the same few float
operations uncontracted, with cos and sin from the host's libm).  The host loops themselves are held to the
numpy restatement in test_orb.py.

The shapes are the smallest at which a level tile (64 x 32 with a 3-pixel halo), the 19-pixel border band, a
multi-level cascade and the wave-per-keypoint grid (4 waves a workgroup) can go wrong."""
import numpy as np
import pytest

from deftri import capi, mapping
from deftri.settings import Settings
import features_ref as fr
from test_orb import PATTERN, SCENES, corner_case, scene

gpu = pytest.mark.gpu
ROUND_TRIPS = 1               # one blocking download of descriptors and status; the upload does not block


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    ctx.orb_set_pattern(PATTERN)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    gpu_ctx.orb_set_pattern(PATTERN)
    return gpu_ctx


def _same(got, want):
    assert got.desc.shape == want.desc.shape and got.desc.tobytes() == want.desc.tobytes()
    assert got.status.tobytes() == want.status.tobytes()
    for k, v in want.report.items():
        if not k.startswith("ms_") and k != "round_trips":
            assert got.report[k] == v, (k, got.report[k], v)


@gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_equals_host_loops(dev, host, name):
    image, p, uv, octave, angle, _ = scene(name)
    for level in range(p["n_scales"]):
        np.testing.assert_array_equal(dev.debug_orb_pyramid(image, p, level), host.debug_orb_pyramid(image, p, level),
                                      err_msg=f"level {level}")
    want = host.orb_describe(image, p, uv, octave, angle)
    got = dev.orb_describe(image, p, uv, octave, angle)
    print(name, {k: v for k, v in got.report.items() if not k.startswith("ms_")})
    _same(got, want)
    assert len(got) > 0 and got.report["round_trips"] == ROUND_TRIPS and want.report["round_trips"] == 0


@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65])
def test_keypoint_counts_off_the_workgroup_size(dev, host, n):
    """4 waves a workgroup, one keypoint a wave: counts that leave waves of the last workgroup without one."""
    image, p, uv, octave, angle, _ = scene("160x120")
    assert len(octave) >= 65
    pick = np.linspace(0, len(octave) - 1, n).astype(int)            # both octaves and hand-placed ones among them
    got = dev.orb_describe(image, p, uv[pick], octave[pick], angle[pick])
    _same(got, host.orb_describe(image, p, uv[pick], octave[pick], angle[pick]))
    assert got.report["round_trips"] == ROUND_TRIPS and got.desc.any()
    none = dev.orb_describe(image, p, uv[:0], octave[:0], angle[:0])
    assert len(none) == 0 and none.report["round_trips"] == 0


@gpu
def test_status_and_pattern_replacement_on_device(gpu_ctx):
    image, p, pattern, uv, octave, angle, _n_fast, _corners, _n_odd = corner_case("200x90_three_scales")
    with capi.Context(-1) as h:
        h.orb_set_pattern(pattern)
        want = h.orb_describe(image, p, uv, octave, angle)
    try:
        gpu_ctx.orb_set_pattern(pattern)
        got = gpu_ctx.orb_describe(image, p, uv, octave, angle)
    finally:
        gpu_ctx.orb_set_pattern(PATTERN)
    _same(got, want)
    assert 0 < got.report["n_outside"] < len(got) and not got.desc[got.status == 1].any()
    with capi.Context(-1) as h:
        h.orb_set_pattern(PATTERN)
        _same(gpu_ctx.orb_describe(image, p, uv, octave, angle), h.orb_describe(image, p, uv, octave, angle))


@gpu
def test_two_sizes_on_one_context_and_strided_image(dev, host):
    """The context's arena grows with the largest call and is reused: a small call, a larger one, the small one
    again, each equal to a fresh context's."""
    small, large = scene("97x83_one_scale"), scene("240x180_realcolon_factor")
    first = dev.orb_describe(*small[:5])
    _same(dev.orb_describe(*large[:5]), host.orb_describe(*large[:5]))
    again = dev.orb_describe(*small[:5])
    _same(again, first)
    with capi.Context(0) as fresh:
        fresh.orb_set_pattern(PATTERN)
        _same(fresh.orb_describe(*large[:5]), host.orb_describe(*large[:5]))
        _same(fresh.orb_describe(*small[:5]), first)
    _same(first, host.orb_describe(*small[:5]))
    image, p, uv, octave, angle, _ = large
    wide = np.zeros((image.shape[0], image.shape[1] + 7), np.uint8)
    wide[:, :image.shape[1]] = image
    _same(dev.orb_describe(wide[:, :image.shape[1]], p, uv, octave, angle), host.orb_describe(image, p, uv, octave, angle))


@gpu
def test_two_frames_to_matches(dev, host):
    """Two frames of one scene (the second with a border mask, so with other keypoints): extractFeatures on both,
    then searchForInitializaion, on the device and on a host-only context."""
    s = Settings(text="FeatureExtractor.nScales: 2\nFeatureExtractor.fScaleFactor: 1.2\nFeatureExtractor.nFeatures: 300\n")
    frames = [fr.make_scene(120, 160, 1, frame=0), fr.make_scene(120, 160, 1, frame=16)]
    grid = dict(cols=16, rows=12, min_col=0.0, min_row=0.0, max_col=160.0, max_row=120.0, n_scales=2, scale_factor=1.2)

    def chain(ctx):
        (k1, d1), (k2, d2) = (mapping.extract_features(ctx, image, s, PATTERN, border) for image, border in frames)
        return k1, d1, k2, d2, ctx.match_for_initialization(grid, k1.uv, k1.octave, d1.desc, k2.uv, k2.octave, d2.desc, 100, 15.0)

    want, got = chain(host), chain(dev)
    assert want[4][3] > 0 and len(want[2]) < len(want[0])
    for a, b in ((got[1], want[1]), (got[3], want[3])):
        _same(a, b)
    for g, w in zip(got[4][:3], want[4][:3]):
        np.testing.assert_array_equal(g, w)
    assert got[4][3] == want[4][3]
