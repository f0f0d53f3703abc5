"""deftri_set_tile_builder on a host-only context: the entry and its refusals, and the device tile
stages reported as not applicable without a device — the plan is then the host's, array for array."""
import numpy as np
import pytest

from deftri import _abi, capi, sim


@pytest.fixture(scope="module")
def host():
    with capi.Context(-1) as c:
        yield c


@pytest.fixture(scope="module")
def problem(host):
    m, _ = sim.simulate_two_view(n=400, seed=3)
    return host.build_graph(m, 1.0, 2e5, np.float32(0.003))


def test_entry_and_abi():
    lib = capi.load()
    assert "deftri_set_tile_builder" in capi.EXPORTED and hasattr(lib, "deftri_set_tile_builder")
    assert lib.deftri_abi_version() == 8


def test_modes(host):
    for bad in (2, -1):
        with pytest.raises(capi.DeftriError) as e:
            host.set_tile_builder(bad)
        assert e.value.code == _abi.DEFTRI_E_ARG
    host.set_tile_builder(1)
    host.set_tile_builder(0)


def test_host_context_builds_on_the_host(host, problem):
    names, want = host.debug_plan_digest(problem, 0, 1)
    host.set_tile_builder(1)
    try:
        names1, got = host.debug_plan_digest(problem, 1, 1)
        info = host.plan_build_info()
    finally:
        host.set_tile_builder(0)
    assert names == names1 and len(got) == 33
    for name, a, b in zip(names, want, got):
        assert a == b, name
    assert (info["builder_used"], info["stages"], info["reason"]) == (0, 0, 1)
