"""findEssentialWithRANSAC with a model per hypothesis and reconstructCameras (deftri_find_essential_ransac,
deftri_reconstruct_cameras) on a host-only context, against the numpy restatements of deftri.matching, and the Python
pieces around them (compute_max_tries, ransac_samples, the report struct).

The conventions are pinned on noise-free correspondences of a known pose pair x2 = R21 x1 + t21 with the fp64
restatement: compute_essential of any eight is +-sqrt(2) [t21]x R21 / |.|_F, and reconstruct_cameras_ref of it returns
R21 and +t21 / |t21|, both to 1e-9.

E_all[h] is held to tol_h = C_TOL * 2^-24 * sigma_1 / sigma_8 (A_h) in the Frobenius norm against the fp64 restatement
(essential_scenes): C_TOL = 0.56 = 4 * 0.14, the largest deviation an error of the float rays causes in the fp64
restatement over the committed cases, in units of 2^-24 sigma_1 / sigma_8, times 4 for rays a last bit or two apart
between libm implementations.  Scores and flags follow the margins_ok convention (essential_scenes.check_ransac).

The issue's prototype reported a tie for the best score (8 and 8) on the case n = 64, seed 1, H = 16; with these
samples the scores there are 35, 11, 8, ... and nothing ties, so the lowest-index rule is exercised on that scene with
its winning sample appended again (the same model at two indices: the tie is asserted)."""
import ctypes as C

import numpy as np
import pytest

from deftri import _abi, capi, mapping, matching
import essential_scenes as es


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


def test_conventions_on_noise_free_rays():
    r1, r2, R21, t21 = es.noise_free_rays(40, 7)
    tx = np.array([[0, -t21[2], t21[1]], [t21[2], 0, -t21[0]], [-t21[1], t21[0], 0]])
    Et = tx @ R21
    Et = np.sqrt(2.0) * Et / np.linalg.norm(Et)
    rng = np.random.default_rng(0)
    for _ in range(8):
        s = rng.choice(40, 8, replace=False)
        E = matching.compute_essential(r1[s], r2[s])
        assert min(np.abs(E - Et).max(), np.abs(E + Et).max()) <= 1e-9
        for flip in (False, True):
            Rg, t, _ = matching.reconstruct_cameras_ref(E, r1, r2, flip_t0=flip)
            assert np.abs(Rg - R21).max() <= 1e-9 and np.abs(t - t21 / np.linalg.norm(t21)).max() <= 1e-9


def test_host_models_on_noise_free_rays(host):
    """The library's closed forms on matches without displaced pixels: under a threshold of 1 rad every hypothesis
    scores every match, and the first is the best."""
    uv1, uv2, k1, k2, *_ = es.ts.scene(64, nans=0, seed=3, offsets=False)
    smp = es.samples(64, 16, 3)
    r = host.find_essential_ransac(uv1, uv2, k1, k2, smp, 1.0)
    assert (r.scores == 64).all() and r.report["best"] == 0 and not r.degenerate.any()


def test_c_tol_is_what_the_restatement_measures():
    c = es.measure_c()
    print("largest deviation in units of 2^-24 sigma_1 / sigma_8:", c)
    assert 4 * c <= es.C_TOL <= 4 * c * 1.1


@pytest.mark.parametrize("key", es.CASES, ids=str)
def test_host_against_restatement(host, key):
    c = es.case(*key)
    r = es.check_ransac(host, c, round_trips=0)
    assert r.report["best"] == c["ref64"]["best"] >= 0
    es.check_cameras(host, c, r)


def test_cameras_recover_the_pose(host):
    """n = 257, seed 2, H = 256: the best model's (Rgood, t) against the true relative pose.  The fp64 restatement
    gives |Rgood - R21|_F = 0.0051 and t . t21 / |t21| = 0.99987 here (the issue's prototype: 0.028 and 0.999); asserted
    with a margin of a factor 2 on the distance from the exact pose (0.0102 and 1 - 2 * 1.3e-4), which is not tighter
    than the prototype's figures allow for the restatement."""
    c = es.case(257, 256, 2, 0)
    r = host.find_essential_ransac(c["uv1"], c["uv2"], c["k1"], c["k2"], c["samples"], es.EPI_TH)
    R21, t21 = es.true_relative_pose(c)
    Rg, t, _ = matching.reconstruct_cameras_ref(r.E, c["r1"], c["r2"], r.inlier)
    pose, _ = host.reconstruct_cameras(c["uv1"], c["uv2"], c["k1"], c["k2"], r.E, r.inlier)
    for R, tt in ((Rg, t), (pose.R.astype(np.float64), pose.t.astype(np.float64))):
        dR, cos = np.linalg.norm(R - R21), float(tt @ t21 / np.linalg.norm(t21))
        print("|Rgood - R21|_F", dR, "t . t21 / |t21|", cos)
        assert dR <= 0.0102 and cos >= 1 - 2.6e-4


def test_tie_takes_the_lowest_index(host):
    c = es.case(64, 16, 1, 0)
    best = c["ref64"]["best"]
    smp = np.concatenate([c["samples"], c["samples"][best:best + 1], c["samples"][best:best + 1, ::-1]])
    r = host.find_essential_ransac(c["uv1"], c["uv2"], c["k1"], c["k2"], smp, es.EPI_TH)
    assert r.scores[16] == r.scores[best] == r.scores.max() and r.scores[17] == r.scores[best]      # a tie is present
    assert r.report["best"] == best < 16
    np.testing.assert_array_equal(r.E_all[16], r.E_all[best])
    # the same winner first: the copy at index 0 now wins
    r0 = host.find_essential_ransac(c["uv1"], c["uv2"], c["k1"], c["k2"], smp[::-1].copy(), es.EPI_TH)
    assert r0.report["best"] == 0 and r0.report["best_score"] == r.report["best_score"]


def test_every_score_zero(host):
    """n = 8, H = 1: the rank-2 projection moves the exact fit and nothing passes 0.003."""
    c = es.case(8, 1, 0, 0)
    assert c["ref64"]["best"] == -1
    r = es.check_ransac(host, c, round_trips=0)
    assert r.report["best"] == -1 and r.report["best_score"] == 0 and not r.inlier.any() and not r.E.any()
    # and a threshold nothing passes
    c = es.case(64, 16, 1, 0)
    r = host.find_essential_ransac(c["uv1"], c["uv2"], c["k1"], c["k2"], c["samples"], 0.0)
    assert r.report["best"] == -1 and not r.scores.any() and not r.inlier.any() and np.isnan(r.err).all()


def test_degenerate_hypotheses(host):
    c = es.case(64, 16, 1, 3)
    args = (c["uv1"], c["uv2"], c["k1"], c["k2"])
    nan_rows = np.flatnonzero(np.isnan(c["uv1"]).any(1))
    assert len(nan_rows) == 3
    smp = c["samples"].copy()
    clean = [h for h in range(16) if not np.isin(smp[h], nan_rows).any()]
    a, b = clean[0], clean[1]
    smp[a, 5] = smp[a, 2]                                     # a repeated index
    smp[b, 7] = nan_rows[0]                                   # a sample through a NaN ray
    r = host.find_essential_ransac(*args, smp, es.EPI_TH)
    ref = matching.find_essential_ransac_ref(c["r1"], c["r2"], smp, es.EPI_TH)
    assert r.degenerate[a] and r.degenerate[b] and r.scores[a] == 0 and r.scores[b] == 0
    np.testing.assert_array_equal(r.degenerate, ref["degenerate"])
    assert r.report["best"] == ref["best"] and r.report["best"] not in (a, b)
    assert r.report["n_degenerate"] == int(r.degenerate.sum())
    # all degenerate: no best
    r = host.find_essential_ransac(*args, np.zeros((3, 8), np.int32), es.EPI_TH)
    assert r.degenerate.all() and r.report["best"] == -1 and r.report["n_degenerate"] == 3
    for bad in (64, -1):                                      # an index out of range
        smp = c["samples"].copy()
        smp[3, 4] = bad
        with pytest.raises(capi.DeftriError, match="outside") as e:
            host.find_essential_ransac(*args, smp, es.EPI_TH)
        assert e.value.code == _abi.DEFTRI_E_ARG
    with pytest.raises(capi.DeftriError, match="fewer than 8") as e:     # n = 7
        host.find_essential_ransac(c["uv1"][:7], c["uv2"][:7], c["k1"], c["k2"], np.arange(8, dtype=np.int32)[None] % 7, es.EPI_TH)
    assert e.value.code == _abi.DEFTRI_E_ARG
    with pytest.raises(capi.DeftriError, match="n_hyp") as e:
        host.find_essential_ransac(*args, np.zeros((0, 8), np.int32), es.EPI_TH)
    assert e.value.code == _abi.DEFTRI_E_ARG
    with pytest.raises(capi.DeftriError, match="singular") as e:
        host.reconstruct_cameras(*args, np.zeros((3, 3), np.float32))
    assert e.value.code == _abi.DEFTRI_E_ARG


def test_cameras_use_mask(host):
    """use = None is every match; the vote counts the used matches only."""
    c = es.case(64, 16, 1, 0)
    E = c["ref64"]["E"].astype(np.float32)
    args = (c["uv1"], c["uv2"], c["k1"], c["k2"], E)
    p_all, a_all = host.reconstruct_cameras(*args)
    p_ones, a_ones = host.reconstruct_cameras(*args, np.ones(64, bool))
    assert a_all == a_ones and np.array_equal(p_all.t, p_ones.t) and abs(a_all) <= 64
    half = np.arange(64) % 2 == 0
    _, a_half = host.reconstruct_cameras(*args, half)
    _, a_rest = host.reconstruct_cameras(*args, ~half)
    # the two halves vote with the same starting t, so their votes add up
    assert a_half + a_rest == a_all
    _, _, aw = matching.reconstruct_cameras_ref(E, c["r1"], c["r2"], half)
    assert a_half == aw
    p0, a0 = host.reconstruct_cameras(c["uv1"][:0], c["uv2"][:0], c["k1"], c["k2"], E)
    assert a0 == 0 and np.array_equal(p0.R, p_all.R)


def test_compute_max_tries():
    assert mapping.compute_max_tries(0.8, 0.95) == 16


def test_ransac_samples():
    c = es.case(257, 65, 2, 0)
    s, labels = mapping.ransac_samples(c["uv1"], 65, 10, return_labels=True)
    s2 = mapping.ransac_samples(c["uv1"], 65, 10)
    assert s.shape == (65, 8) and s.dtype == np.int32 and np.array_equal(s, s2)
    assert not np.array_equal(s, mapping.ransac_samples(c["uv1"], 65, 11))
    assert s.min() >= 0 and s.max() < 257
    assert (np.sort(labels[s], 1) == np.arange(8)).all()                 # eight distinct clusters per row
    assert len(np.unique(s)) > 8                                          # and not the same draw every time
    s8 = mapping.ransac_samples(c["uv1"][:8], 4, 10)
    assert (np.sort(s8, 1) == np.arange(8)).all()                         # 8 points: one per cluster
    with pytest.raises(ValueError):
        mapping.ransac_samples(c["uv1"][:7], 4, 10)


def test_abi():
    lib = capi.load()
    assert lib.deftri_abi_version() == 8
    assert lib.deftri_sizeof(22) == C.sizeof(_abi.EssentialReport) == 56
    for name in ("deftri_find_essential_ransac", "deftri_reconstruct_cameras"):
        assert name in capi.EXPORTED and hasattr(lib, name)
