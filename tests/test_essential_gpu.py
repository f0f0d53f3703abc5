"""findEssentialWithRANSAC with a model per hypothesis (k_rays, k_essential_models, k_score, k_best) and
reconstructCameras (k_camera_vote) on the device: against the library's host-only context, against the numpy
restatements with the assertions of test_essential (essential_scenes.check_ransac / check_cameras), prefixes of one
call against another, and mapping.reconstruct_environment end to end.

Shapes: n = 257 crosses the 256-thread block, H = 65 a wave of hypotheses in k_essential_models and the 64-hypothesis
tile of k_score, (8, 1) is the smallest call and scores nothing.

Scores, best, inlier, degenerate and away are integers and equal the host's wherever the two contexts' E_all[h] agree
bit for bit (the model arithmetic is + - * / sqrt in fp64 without contraction on both; the rays go through sinf /
cosf of two libm's).  Where a model differs, E_all is compared through tol_h and the scores through the margin rule;
the test prints how many hypotheses that concerns."""
import numpy as np
import pytest

from conftest import GOLDEN
from deftri import capi, mapping, sim
from deftri.mapmodel import KeyFrame, Map, SE3f
from deftri.settings import Settings
import depth_image_ref as ref
import essential_scenes as es
import matching_scenes as ms
import triangulation_scene as ts

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


def _call(ctx, c, samples=None, n=None):
    n = c["n"] if n is None else n
    return ctx.find_essential_ransac(c["uv1"][:n], c["uv2"][:n], c["k1"], c["k2"], c["samples"] if samples is None else samples,
                                     es.EPI_TH)


@gpu
@pytest.mark.parametrize("shape", es.GPU_SHAPES, ids=str)
def test_device_against_host_context(gpu_ctx, host, shape):
    c = es.case(*shape)
    d, h = _call(gpu_ctx, c), _call(host, c)
    same = (d.E_all.view(np.uint32) == h.E_all.view(np.uint32)).all((1, 2))
    print(shape, "models bit-identical to the host's:", int(same.sum()), "of", c["H"], "device report", d.report)
    np.testing.assert_array_equal(d.degenerate, h.degenerate)
    np.testing.assert_array_equal(d.scores[same], h.scores[same])
    ok = ~d.degenerate
    dE = np.linalg.norm((d.E_all.astype(np.float64) - h.E_all).reshape(c["H"], 9), axis=1)
    assert (dE[ok] <= es.tol(c)[ok]).all()
    near = es.near_threshold(d.E_all, c) + es.near_threshold(h.E_all, c)
    assert (np.abs(d.scores - h.scores) <= near).all()
    assert d.report["round_trips"] == 1 and h.report["round_trips"] == 0
    if same.all():
        assert d.report["best"] == h.report["best"] and d.report["best_score"] == h.report["best_score"]
        np.testing.assert_array_equal(d.E.view(np.uint32), h.E.view(np.uint32))
        if d.report["best"] >= 0:
            # the errors go through acosf of two libm's: the mask is equal off the threshold
            far = np.abs(h.err.astype(np.float64) - es.EPI_TH) > 1e-3 * es.EPI_TH
            np.testing.assert_array_equal(d.inlier[far], h.inlier[far])
            assert np.abs(d.err - h.err).max() <= 2e-6
            pd, ad = gpu_ctx.reconstruct_cameras(c["uv1"], c["uv2"], c["k1"], c["k2"], h.E, h.inlier)
            ph, ah = host.reconstruct_cameras(c["uv1"], c["uv2"], c["k1"], c["k2"], h.E, h.inlier)
            assert ad == ah and np.array_equal(pd.R, ph.R) and np.array_equal(pd.t, ph.t)
        else:
            assert not d.inlier.any() and np.isnan(d.err).all()


@gpu
@pytest.mark.parametrize("key", es.CASES + [(8, 1, 0, 0)], ids=str)
def test_device_against_restatement(gpu_ctx, key):
    c = es.case(*key)
    r = es.check_ransac(gpu_ctx, c, round_trips=1)
    assert r.report["best"] == c["ref64"]["best"]
    if r.report["best"] >= 0:
        es.check_cameras(gpu_ctx, c, r)


@gpu
def test_tie_and_degenerate_on_device(gpu_ctx, host):
    c = es.case(64, 16, 1, 3)
    best = c["ref64"]["best"]
    smp = np.concatenate([c["samples"], c["samples"][best:best + 1], np.zeros((1, 8), np.int32)])
    d, h = _call(gpu_ctx, c, smp), _call(host, c, smp)
    assert d.scores[16] == d.scores[best] == d.scores.max() and d.report["best"] == best          # a tie, the lowest index
    assert d.degenerate[17] and d.degenerate.sum() == h.degenerate.sum() == d.report["n_degenerate"] >= 2
    np.testing.assert_array_equal(d.degenerate, h.degenerate)
    smp[2, 3] = 64
    with pytest.raises(capi.DeftriError, match="outside"):
        _call(gpu_ctx, c, smp)
    with pytest.raises(capi.DeftriError, match="fewer than 8"):
        _call(gpu_ctx, c, smp[:1] % 7, n=7)
    z = gpu_ctx.find_essential_ransac(c["uv1"], c["uv2"], c["k1"], c["k2"], c["samples"], 0.0)
    assert z.report["best"] == -1 and not z.scores.any() and not z.inlier.any() and not z.E.any() and np.isnan(z.err).all()


@gpu
@pytest.mark.parametrize("k", [1, 64, 65])
def test_hypothesis_prefix_is_bit_identical(gpu_ctx, k):
    """A hypothesis is one thread's model and its own counter: samples[:k] gives rows [:k] of the call on all 256."""
    c = es.case(257, 256, 2, 0)
    full, part = _call(gpu_ctx, c), _call(gpu_ctx, c, c["samples"][:k])
    np.testing.assert_array_equal(part.E_all.view(np.uint32), full.E_all[:k].view(np.uint32))
    np.testing.assert_array_equal(part.scores, full.scores[:k])
    np.testing.assert_array_equal(part.degenerate, full.degenerate[:k])


@gpu
def test_match_prefix_is_bit_identical(gpu_ctx):
    """A match's error is one thread's work: the first 8 matches under a hypothesis drawn from them reproduce err[:8] of
    the call on all 257 under the same single hypothesis."""
    c = es.case(257, 256, 2, 0)
    smp = np.arange(8, dtype=np.int32)[None, ::-1].copy()
    full, part = _call(gpu_ctx, c, smp), _call(gpu_ctx, c, smp, n=8)
    np.testing.assert_array_equal(part.E_all.view(np.uint32), full.E_all.view(np.uint32))
    if full.report["best"] == 0 and part.report["best"] == 0:
        np.testing.assert_array_equal(part.err.view(np.uint32), full.err[:8].view(np.uint32))
        np.testing.assert_array_equal(part.inlier, full.inlier[:8])
    else:                                                     # no inlier among the first 8: the score of the full call decides
        assert part.report["best"] == -1 and not full.inlier[:8].any()
    # with a threshold every match passes, both calls have a best and the errors are comparable
    full = gpu_ctx.find_essential_ransac(c["uv1"], c["uv2"], c["k1"], c["k2"], smp, 4.0)
    part = gpu_ctx.find_essential_ransac(c["uv1"][:8], c["uv2"][:8], c["k1"], c["k2"], smp, 4.0)
    assert full.report["best"] == part.report["best"] == 0 and part.report["best_score"] == 8
    np.testing.assert_array_equal(part.err.view(np.uint32), full.err[:8].view(np.uint32))


# ---- end to end: two keyframes over 64 x 64 depth images, the second without a pose ----
N_REAL = 200
YAML_TAIL = ("\nCamera.cols: 64\nCamera.rows: 64\nFeatureGrid.nGridCols: 8\nFeatureGrid.nGridRows: 8\n"
             "FeatureExtractor.nFeatures: 200\nFeatureExtractor.nScales: 8\nFeatureExtractor.fScaleFactor: 1.2\n"
             "Matching.initialization: 50\nMatching.initialization.radius: 40\nTriangulation.minMatches: 30\n"
             "Triangulation.depthLimit: 100.0\n")


def _settings():
    base = (GOLDEN / "sim_default" / "settings.yaml").read_text().splitlines()
    return Settings(text="\n".join(ln for ln in base if not ln.startswith(("Camera.k", "Camera.p"))) + YAML_TAIL)


def _pair():
    """The 64 x 64 pair of the matching tests' shape, the reference keyframe at the origin and the current one without a
    pose of its own (the identity), and the true matches."""
    uv1, uv2, k1, k2, _, _, info = ts.scene(N_REAL, seed=1, kb8_1=ts.KB8_SMALL_1, kb8_2=ts.KB8_SMALL_2, offsets=False, nans=0)
    rng = np.random.default_rng(3)
    perm = rng.permutation(N_REAL)
    kp2 = np.zeros_like(uv2); z2 = np.zeros(N_REAL)
    kp2[perm] = uv2; z2[perm] = info["z2"]
    d1 = rng.integers(0, 256, (N_REAL, 32), dtype=np.uint8)
    d2 = np.zeros_like(d1)
    for i in range(N_REAL):
        d2[perm[i]] = ms.flip_bits(d1[i], rng.choice(256, rng.integers(0, 10), replace=False))
    inv_s2 = sim.inv_sigma2_table(8, 1.2)
    kf_ref = KeyFrame(0, SE3f(), k1, N_REAL, inv_s2, uv1, np.zeros(N_REAL, np.int32), info["z1"], descriptors=d1)
    kf_cur = KeyFrame(1, SE3f(), k2, N_REAL, inv_s2, kp2, np.zeros(N_REAL, np.int32), z2, descriptors=d2)
    m = Map()
    m.insert_keyframe(kf_ref); m.insert_keyframe(kf_cur)
    ref.synthetic_images(m, (64, 64), seed=5)
    return kf_ref, kf_cur, perm.astype(np.int64)


def _snapshot(m, kf_ref, kf_cur):
    slots = [[None if mp is None else (mp.id, tuple(np.asarray(mp.position).tolist())) for mp in kf.map_points]
             for kf in (kf_ref, kf_cur)]
    return {"slots": slots, "ids": sorted(m.map_points), "obs": {k: dict(v) for k, v in m.kf_obs.items()},
            "scales": (kf_ref.estimated_depth_scale, kf_cur.estimated_depth_scale)}


def _reset(kf_ref, kf_cur):
    for kf in (kf_ref, kf_cur):
        kf.map_points = [None] * N_REAL
        kf.estimated_depth_scale = 1.0
    kf_cur.pose = SE3f()


@gpu
def test_reconstruct_environment(gpu_ctx):
    kf_ref, kf_cur, matches = _pair()
    matches[::7] = -1                                         # some reference keypoints without a match
    st = _settings()
    st.epipolar_th = 0.01
    idx = np.flatnonzero(matches >= 0)
    uv1, uv2 = kf_ref.keypoints[idx], kf_cur.keypoints[matches[idx]]
    samples = mapping.ransac_samples(uv1, 16, seed=10)
    try:
        # by hand: the two Context methods, then monocular_map_initialization
        res = gpu_ctx.find_essential_ransac(uv1, uv2, kf_ref.kb8, kf_cur.kb8, samples, st.epipolar_th)
        assert res.report["best"] >= 0 and res.report["best_score"] > 100
        pose, away = gpu_ctx.reconstruct_cameras(uv1, uv2, kf_ref.kb8, kf_cur.kb8, res.E, res.inlier)
        fed = matches.copy()
        fed[idx[~res.inlier]] = -1
        kf_cur.pose = pose
        m1, rep1 = mapping.monocular_map_initialization(gpu_ctx, kf_ref, kf_cur, fed, st)
        assert m1 is not None and rep1["accepted"] == 1 and rep1["n_map_points"] > 50
        want = _snapshot(m1, kf_ref, kf_cur)
        _reset(kf_ref, kf_cur)
        start = kf_cur.pose
        m2, rep2 = mapping.reconstruct_environment(gpu_ctx, kf_ref, kf_cur, matches, st, samples=samples)
        assert m2 is not None and _snapshot(m2, kf_ref, kf_cur) == want
        assert rep2["n_inliers"] == res.report["best_score"] and rep2["best"] == res.report["best"] and rep2["away"] == away
        assert {k: v for k, v in rep2.items() if k in rep1} == rep1 and rep2["n_matches"] == len(idx)
        assert kf_cur.pose is not start and np.array_equal(kf_cur.pose.R, pose.R) and np.array_equal(kf_cur.pose.t, pose.t)
        assert np.array_equal(kf_ref.pose.R, np.eye(3, dtype=np.float32))
        # the default samples: seeded, so twice the same
        _reset(kf_ref, kf_cur)
        m3, rep3 = mapping.reconstruct_environment(gpu_ctx, kf_ref, kf_cur, matches, st, seed=10)
        pose3 = kf_cur.pose
        _reset(kf_ref, kf_cur)
        m4, rep4 = mapping.reconstruct_environment(gpu_ctx, kf_ref, kf_cur, matches, st, seed=10)
        assert rep3["n_hypotheses"] == 16 and (m3 is None) == (m4 is None) and rep3["n_inliers"] == rep4["n_inliers"]
        assert np.array_equal(pose3.R, kf_cur.pose.R)
        # a threshold of 0: no map, and the pose is restored
        _reset(kf_ref, kf_cur)
        start = kf_cur.pose
        st.epipolar_th = 0.0
        m5, rep5 = mapping.reconstruct_environment(gpu_ctx, kf_ref, kf_cur, matches, st, samples=samples)
        assert m5 is None and rep5["n_inliers"] == 0 and rep5["best"] == -1 and kf_cur.pose is start
        # reconstructPoints refuses the pair: the pose is restored as well
        st.epipolar_th = 0.01
        st.depth_limit = 1e-6
        m6, rep6 = mapping.reconstruct_environment(gpu_ctx, kf_ref, kf_cur, matches, st, samples=samples)
        assert m6 is None and rep6["accepted"] == 0 and kf_cur.pose is start
    finally:
        gpu_ctx.set_depth_images([])
