"""deftri_set_graph_builder / deftri_graph_build_info on a host-only context: the entries and their
refusals, the info before any build, and no effect without a device — the graph is the host build's in every field
and the info says `not applicable`.  tests/test_graph_builder_gpu.py compares the device stages on a device."""
import numpy as np
import pytest

from deftri import _abi, capi, sim

W = (1.0, 2e5, np.float32(0.003))
FIELDS = ("points", "tg", "scales", "cam_kb8", "cam_pose", "rep_point", "rep_cam", "rep_obs", "rep_info",
          "dep_point", "dep_scale", "dep_cam", "dep_meas", "dep_info", "arap_pts", "arap_pair", "arap_rot",
          "arap_w", "rot", "pair_area", "pair_info", "order_xy", "point_ids")


def test_entries_and_abi():
    lib = capi.load()
    for name in ("deftri_set_graph_builder", "deftri_graph_build_info"):
        assert name in capi.EXPORTED and hasattr(lib, name)
    assert lib.deftri_abi_version() == 8


def test_modes():
    with capi.Context(-1) as host:
        for bad in (2, -1):
            with pytest.raises(capi.DeftriError) as e:
                host.set_graph_builder(bad)
            assert e.value.code == _abi.DEFTRI_E_ARG
        host.set_graph_builder(1)
        host.set_graph_builder(0)


def test_info_is_zero_before_a_build():
    with capi.Context(-1) as host:
        assert host.graph_build_info() == dict(builder_used=0, stages=0, reason=0, ms=0.0)
        host.set_graph_builder(1)
        assert host.graph_build_info() == dict(builder_used=0, stages=0, reason=0, ms=0.0)


def test_no_effect_on_a_host_context():
    m, _ = sim.simulate_two_view(n=400, seed=3)
    with capi.Context(-1) as a, capi.Context(-1) as b:
        want = a.build_graph(m, *W)
        b.set_graph_builder(1)
        got = b.build_graph(m, *W)
        info = b.graph_build_info()
        info0 = a.graph_build_info()
        for f in FIELDS:
            assert np.array_equal(getattr(want, f), getattr(got, f)), f
        assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 1)
        assert info["ms"] > 0
        assert (info0["builder_used"], info0["stages"], info0["reason"]) == (0, 0, 0)
        # a memo hit leaves the info of the last full build in place
        b.build_graph(m, *W)
        assert b.graph_stats()[0] == 1 and b.graph_build_info() == info
