"""deftri_set_multi_pair_builder on a host-only context: the entry and its refusals, ABI 8, and the
device stages of a multi-pair plan reported as not applicable without a device — the plan is then the host's."""
import numpy as np
import pytest

from deftri import _abi, capi, sim

W = (1.0, 1e7, np.float32(0.3))


@pytest.fixture(scope="module")
def host():
    with capi.Context(-1) as c:
        yield c


@pytest.fixture(scope="module")
def problem(host):
    p = host.build_graph(sim.multi_view_arrays(n=60, k=4), *W)
    assert p.n_pairs == 6 and p.n_scales == 12
    return p


def test_entry_and_abi():
    lib = capi.load()
    assert "deftri_set_multi_pair_builder" in capi.EXPORTED and hasattr(lib, "deftri_set_multi_pair_builder")
    assert lib.deftri_abi_version() == 8


def test_other_modes_are_refused(host):
    for mode in (2, -1):
        with pytest.raises(capi.DeftriError) as e:
            host.set_multi_pair_builder(mode)
        assert e.value.code == _abi.DEFTRI_E_ARG
    host.set_multi_pair_builder(1)
    host.set_multi_pair_builder(0)
    # a switch of its own: the plan builder keeps its two modes
    with pytest.raises(capi.DeftriError) as e:
        host.set_plan_builder(2)
    assert e.value.code == _abi.DEFTRI_E_ARG


def test_host_context_builds_on_the_host(host, problem):
    names, want = host.debug_plan_digest(problem, 0, 1)
    assert dict(zip(names, want))["tile_tab"] != 1469598103934665603        # the multi-pair tile layout was built
    host.set_multi_pair_builder(1)
    host.set_layout_builder(1)
    try:
        _, got = host.debug_plan_digest(problem, 1, 1)
        info = host.plan_build_info()
        stats = host.debug_plan_layout_stats(problem, 1, 1)
    finally:
        host.set_multi_pair_builder(0)
        host.set_layout_builder(0)
    for name, a, b in zip(names, want, got):
        assert a == b, name
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 1)
    assert stats == host.debug_plan_layout_stats(problem, 0, 1)
