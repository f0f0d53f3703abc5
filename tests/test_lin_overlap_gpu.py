"""The iterative plan's linearization with the row pass and the heavy vertices' block partials in one
launch (k_sp_glin): b and the Hessian diagonal against the oracle, at the smallest shapes that reach
every branch of the launch —

  tv700    two views, 700 correspondences (~4k ARAP edges): more than one group of kSpGlinGroup
           blocks, waves with lane pairs (wsplit);
  tv6000   two views, 6000 correspondences (~36k ARAP edges): more than kSpHeavyChunk = 128 block
           partials, so T_g's sums span two chunks of k_sp_glin_heavy (the vertex ticket);
  mv8      8 keyframes, all 28 pairs (56 scales): several heavy vertices, depth blocks, the
           multi-pair row path.

The tolerance is test_iterative_gradient_and_solve_match_oracle's (1e-13 relative, fp64 sums of a few
thousand terms in another order).  deftri_eval_gradient linearizes with analytic Jacobians on this
plan; the numeric (g2o) Jacobians are reached through solve_lm(analytic=False), whose state the
gradient is then checked at, and whose chi2 history must repeat bit for bit."""
import copy

import numpy as np
import pytest

from deftri import capi, sim
from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = 1e-13


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def _tv(n):
    m, _ = sim.simulate_two_view(n=n, seed=2, scale_scene=True, compact=True)
    host = capi.Context(-1)
    p = host.build_graph(m, 1.0, 2e5, np.float32(0.003))
    host.close()
    return p


def _mv():
    m, _ = sim.simulate_multi_view(n=100, k=8, seed=1)
    host = capi.Context(-1)
    p = host.build_graph(m, 1.0, 1e7, np.float32(0.3))
    host.close()
    return p


def oracle_b_diag(p):
    """b and diag(H) of the oracle's analytic linearization at p's state, without a dense H."""
    b, _, _ = oracle.linearize(p, analytic=True)
    ri, ci, v = oracle.hessian_coo(p, analytic=True)
    d = np.zeros(p.n_unknowns)
    on = ri == ci
    np.add.at(d, ri[on], v[on])
    return b, d


_cache = {}


@pytest.fixture(params=["tv700", "tv6000", "mv8"])
def case(request):
    """(problem, oracle b, oracle diagonal) of a shape: built once, shared, never written."""
    k = request.param
    if k not in _cache:
        p = {"tv700": lambda: _tv(700), "tv6000": lambda: _tv(6000), "mv8": _mv}[k]()
        lo, hi, pairs = {"tv700": (8 * 256, 128 * 256, 1), "tv6000": (128 * 256, 1 << 30, 1), "mv8": (0, 1 << 30, 28)}[k]
        assert lo < len(p.arap_pair) < hi and p.n_pairs == pairs      # the branches the shape is here for
        _cache[k] = (p,) + oracle_b_diag(p)
    return _cache[k]


@pytest.fixture
def it_ctx(gpu_ctx):
    gpu_ctx.set_plan("iterative")
    gpu_ctx.set_linear_solver("pcg", max_iterations=4096)
    yield gpu_ctx
    gpu_ctx.set_plan("multifrontal")
    gpu_ctx.set_linear_solver("pcg")


def test_gradient_matches_oracle(it_ctx, case):
    p, b_ref, d_ref = case
    it_ctx.upload(p)
    assert it_ctx.plan_info()["plan"] == "iterative"
    b, d = it_ctx.gradient()
    print(f"rel b {rel(b, b_ref):.3e}  rel diag {rel(d, d_ref):.3e}")
    assert rel(b, b_ref) < TOL and rel(d, d_ref) < TOL


def test_gradient_twice_identical_bits(it_ctx, case):
    """Tickets and counters of the linearization are back at zero after a launch."""
    p = case[0]
    it_ctx.upload(p)
    b1, d1 = it_ctx.gradient()
    b2, d2 = it_ctx.gradient()
    assert np.array_equal(b1, b2) and np.array_equal(d1, d2)


def test_gradient_after_numeric_lm_and_reset(it_ctx, case):
    """upload -> gradient; solve_lm(3, numeric J) -> gradient against the oracle at the downloaded
    state; reset_state -> the first gradient's bits; and the numeric LM run repeats bit for bit."""
    p, b_ref, d_ref = case
    it_ctx.upload(p)
    b0, d0 = it_ctx.gradient()
    assert rel(b0, b_ref) < TOL and rel(d0, d_ref) < TOL
    r1 = it_ctx.solve_lm(3, analytic=False)
    q = copy.copy(p)
    pts, sc, tg = it_ctx.download()
    q.points, q.scales, q.tg = pts, sc, tg
    bq_ref, dq_ref = oracle_b_diag(q)
    bq, dq = it_ctx.gradient()
    print(f"after LM: rel b {rel(bq, bq_ref):.3e}  rel diag {rel(dq, dq_ref):.3e}")
    assert rel(bq, bq_ref) < TOL and rel(dq, dq_ref) < TOL
    it_ctx.reset_state()
    b1, d1 = it_ctx.gradient()
    assert np.array_equal(b0, b1) and np.array_equal(d0, d1)
    r2 = it_ctx.solve_lm(3, analytic=False)
    assert r1["chi2_iter"] == r2["chi2_iter"] and r1["trials_iter"] == r2["trials_iter"]
