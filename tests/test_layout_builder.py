"""deftri_set_layout_builder on a host-only context: the entry and its refusals, no effect without a
device, and deftri_debug_plan_layout_stats — the figures of the host's phase-1 blocks and wave layout on the scenes
tests/test_layout_builder_gpu.py compares on the device, which show that those scenes hold the cases that test
claims to cover (split and unsplit waves, a look-ahead across two sort windows, two depth blocks per scale)."""
import ctypes as C

import numpy as np
import pytest

from deftri import _abi, capi, sim

W = (1.0, 2e5, np.float32(0.003))


@pytest.fixture(scope="module")
def host():
    with capi.Context(-1) as c:
        yield c


@pytest.fixture(scope="module")
def cloud():
    """The compacted two-view scene of tests/test_tile_builder_gpu.py: a prefix is a scene of that many correspondences."""
    _, gt = sim.simulate_two_view(n=3200, seed=11, compact=True)
    assert len(gt["original"]) >= 2049
    return gt["original"], gt["moved"]


def graph_of(host, cloud, n):
    orig, moved = cloud
    m, gt = sim.simulate_two_view(orig=orig[:n], moved=moved[:n], compact=True)
    assert len(gt["original"]) == n and gt["valid"].all()
    p = host.build_graph(m, *W)
    assert p.n_points == 2 * n and p.n_pairs == 1
    return p


def test_entries_and_abi():
    lib = capi.load()
    for name in ("deftri_set_layout_builder", "deftri_debug_plan_layout_stats"):
        assert name in capi.EXPORTED and hasattr(lib, name)
    assert lib.deftri_abi_version() == 8


def test_modes(host):
    for bad in (2, -1):
        with pytest.raises(capi.DeftriError) as e:
            host.set_layout_builder(bad)
        assert e.value.code == _abi.DEFTRI_E_ARG
    host.set_layout_builder(1)
    host.set_layout_builder(0)


def test_no_effect_on_a_host_context(host, cloud):
    p = graph_of(host, cloud, 300)
    names, want = host.debug_plan_digest(p, 0, 1)
    stats = host.debug_plan_layout_stats(p, 0, 1)
    host.set_plan_builder(1)
    host.set_tile_builder(1)
    host.set_layout_builder(1)
    try:
        names1, got = host.debug_plan_digest(p, 1, 1)
        info = host.plan_build_info()
        stats1 = host.debug_plan_layout_stats(p, 1, 1)
        info1 = host.plan_build_info()
    finally:
        host.set_layout_builder(0)
        host.set_tile_builder(0)
        host.set_plan_builder(0)
    assert names == names1 and want == got and stats == stats1
    for i in (info, info1):
        assert (i["builder_used"], i["stages"], i["reason"]) == (0, 0, 1)


def test_stats_small_buffer_and_mode(host, cloud):
    p = graph_of(host, cloud, 64)
    d = p.to_desc()
    out = np.zeros(8, np.int64)
    ptr = out.ctypes.data_as(C.POINTER(C.c_int64))
    assert host.lib.deftri_debug_plan_layout_stats(host.h, C.byref(d), 0, 1, ptr, 7) == _abi.DEFTRI_E_ARG
    assert host.lib.deftri_debug_plan_layout_stats(host.h, C.byref(d), 2, 1, ptr, 8) == _abi.DEFTRI_E_ARG


# the host build's figures (waves, split, two-window look-ahead, zero-step, slot steps, blocks, depth blocks, largest
# heavy run) of the prefixes, as deftri_debug_plan_layout_stats(p, 0, 1) reports them
HOST_FIGURES = {
    300: (12, 5, 1, 0, 133, 11, 4, 7),
    1024: (37, 10, 1, 0, 439, 32, 8, 24),
    2049: (78, 26, 5, 0, 900, 66, 18, 48),
}


@pytest.mark.parametrize("n", [300, 1024, 2049])
def test_prefixes_hold_the_cases(host, cloud, n):
    """Every named size has every case: split and unsplit waves; a wave whose 64-row look-ahead covers rows of two
    sort windows (asked from 1024 on; 300 — 600 rows — has one too); two depth blocks per scale (from 257 on)."""
    p = graph_of(host, cloud, n)
    s = host.debug_plan_layout_stats(p, 0, 1)
    assert tuple(s[k] for k in capi.PLAN_LAYOUT_STATS) == HOST_FIGURES[n], s
    assert s["split_waves"] > 0 and s["waves"] - s["split_waves"] > 0
    if n >= 1024:
        assert s["two_window_waves"] > 0
    assert s["depth_blocks"] >= 2 * p.n_scales and p.n_scales == 2
    # the waves cover the own rows: a split wave takes 32 of them, another 64, the last what is left
    rows = 2 * n
    assert 32 * s["split_waves"] + 64 * (s["waves"] - s["split_waves"]) >= rows
    assert s["blocks"] - s["depth_blocks"] == -(-len(p.arap_pts) // 256)
    assert s["max_heavy_run"] == max(s["blocks"] - s["depth_blocks"], s["depth_blocks"] // 2)
