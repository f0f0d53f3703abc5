"""deftri_set_multi_tile_builder and deftri_debug_plan_tile_digest on a host-only context: the entries and
their refusals, ABI 8, the device stages reported as not applicable without a device — the plan is then the host's —
and the tile digest over the arrays only a multi-pair tile plan holds."""
import numpy as np
import pytest

from deftri import _abi, capi, sim

W = (1.0, 1e7, np.float32(0.3))
FNV_BASIS = 1469598103934665603          # the digest of an empty array
SWITCHES = ("set_plan_builder", "set_tile_builder", "set_layout_builder", "set_multi_pair_builder", "set_multi_tile_builder")
ARRAYS = ("tile_trow", "tile_tdst", "tile_poff", "tile_nshare")


@pytest.fixture(scope="module")
def host():
    with capi.Context(-1) as c:
        yield c


@pytest.fixture(scope="module")
def problem(host):
    p = host.build_graph(sim.multi_view_arrays(n=60, k=4), *W)
    assert p.n_pairs == 6 and p.n_scales == 12
    return p


def test_entries_and_abi():
    lib = capi.load()
    for name in ("deftri_set_multi_tile_builder", "deftri_debug_plan_tile_digest"):
        assert name in capi.EXPORTED and hasattr(lib, name)
    assert lib.deftri_abi_version() == 8
    assert capi.PLAN_TILE_DIGEST_NAMES == ARRAYS + ("tile_scalars", "combined")


def test_other_modes_are_refused(host):
    for mode in (2, -1):
        with pytest.raises(capi.DeftriError) as e:
            host.set_multi_tile_builder(mode)
        assert e.value.code == _abi.DEFTRI_E_ARG
    host.set_multi_tile_builder(1)
    host.set_multi_tile_builder(0)


def test_host_context_builds_on_the_host(host, problem):
    names, want = host.debug_plan_digest(problem, 0, 1)
    tnames, twant = host.debug_plan_tile_digest(problem, 0, 1)
    assert len(want) == 33 and len(twant) == 6
    for f in SWITCHES[1:]:
        getattr(host, f)(1)
    try:
        _, got = host.debug_plan_digest(problem, 1, 1)
        info = host.plan_build_info()
        _, tgot = host.debug_plan_tile_digest(problem, 1, 1)
        tinfo = host.plan_build_info()
    finally:
        for f in SWITCHES:
            getattr(host, f)(0)
    for name, a, b in zip(names + tnames, want + twant, got + tgot):
        assert a == b, name
    for i in (info, tinfo):
        assert (i["builder_used"], i["stages"], i["reason"]) == (0, 0, 1)
    t = dict(zip(tnames, twant))
    for name in ARRAYS:
        assert t[name] != FNV_BASIS, name


def test_one_pair_plan_has_none_of_the_arrays(host):
    m, _ = sim.simulate_two_view(n=300, seed=3, compact=True)
    one = host.build_graph(m, 1.0, 2e5, np.float32(0.003))
    assert one.n_pairs == 1
    assert dict(zip(*host.debug_plan_digest(one, 0, 1)))["tile_tab"] != FNV_BASIS
    t = dict(zip(*host.debug_plan_tile_digest(one, 0, 1)))
    for name in ARRAYS:
        assert t[name] == FNV_BASIS, name
    assert t["tile_scalars"] != FNV_BASIS


def test_too_little_room_is_refused(host, problem):
    import ctypes as C
    d = problem.to_desc()
    out = np.zeros(5, np.uint64)
    n = C.c_int32(0)
    rc = host.lib.deftri_debug_plan_tile_digest(host.h, C.byref(d), 0, 1, out.ctypes.data_as(C.POINTER(C.c_uint64)), 5, C.byref(n))
    assert rc == _abi.DEFTRI_E_ARG
