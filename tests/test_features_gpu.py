"""deftri_fast_extract on the device (k_resize, k_fast_cells, k_mask_rows / k_mask_cols, k_keypoints) against
the library's sequential host loops on a host-only context: every output array bit for bit, angles included
(both sides run the same float operations uncontracted), every count of the report, and the two stages the
debug entries expose.  The host loops themselves are held to the numpy restatement in test_features.py.

The shapes are the smallest at which a cell tile, a clipped last cell, a multi-level pyramid and the order of
the compacted candidates can go wrong."""
import numpy as np
import pytest

from deftri import capi
import features_ref as fr
from test_features import ARRAYS, SCENES, scene

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


def _same(got, want):
    for k in ARRAYS:
        g, w = getattr(got, k), getattr(want, k)
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert g.tobytes() == w.tobytes(), k
    for k, v in want.report.items():
        if not k.startswith("ms_") and k != "round_trips":
            assert got.report[k] == v, (k, got.report[k], v)


@gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_equals_host_loops(gpu_ctx, host, name):
    image, border, p = scene(name)
    want = host.fast_extract(image, p, border)
    got = gpu_ctx.fast_extract(image, p, border)
    print(name, {k: v for k, v in got.report.items() if k.startswith("n_") or k == "round_trips"})
    _same(got, want)
    assert len(got) > 0 and got.report["round_trips"] == 2


@gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_stages_equal_host_loops(gpu_ctx, host, name):
    image, _border, p = scene(name)
    for level in range(p["n_scales"]):
        np.testing.assert_array_equal(gpu_ctx.debug_fast_pyramid(image, p, level), host.debug_fast_pyramid(image, p, level))
        got, want = gpu_ctx.debug_fast_candidates(image, p, level), host.debug_fast_candidates(image, p, level)
        assert len(want[0]) > 0
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


@gpu
def test_repeated_call_and_two_sizes_on_one_context(gpu_ctx, host):
    """No state survives a call: the same image twice, then another size, then the first again."""
    a, b = scene("240x180_realcolon_factor"), scene("97x83_one_scale")
    first = gpu_ctx.fast_extract(a[0], a[2], a[1])
    _same(gpu_ctx.fast_extract(a[0], a[2], a[1]), first)
    _same(gpu_ctx.fast_extract(b[0], b[2], b[1]), host.fast_extract(b[0], b[2], b[1]))
    _same(gpu_ctx.fast_extract(a[0], a[2], a[1]), first)
    _same(first, host.fast_extract(a[0], a[2], a[1]))


@gpu
def test_device_mask_reads_and_strided_image(gpu_ctx, host):
    rng = np.random.default_rng(5)
    image, _ = fr.make_scene(260, 300, 7, n_blobs=2)
    border = np.zeros_like(image)
    border[:, :3] = 1; border[-2:, :] = 200
    for level in (0, 3, 5):
        xy = np.stack([rng.integers(0, 300, 1000), rng.integers(0, 260, 1000)], 1).astype(np.int32)
        want = host.debug_fast_mask(image, level, xy, border)
        np.testing.assert_array_equal(gpu_ctx.debug_fast_mask(image, level, xy, border), want)
        assert want.any() and not want.all()
    img, bm, p = scene("border_mask")
    wide = np.zeros((img.shape[0], img.shape[1] + 7), np.uint8)
    wide[:, :img.shape[1]] = img
    _same(gpu_ctx.fast_extract(wide[:, :img.shape[1]], p, bm), host.fast_extract(img, p, bm))
