"""TEST INFRASTRUCTURE ONLY: scenes, samples and bounds of the essential-matrix tests (seeded numpy, on
triangulation_scene.scene).

A case is (n, H, seed, nans): triangulation_scene.scene(n, nans=nans, seed=seed), whose correspondences are a
fifth to a third displaced by 6-10 px, and H samples drawn by one default_rng(seed), choice(n, 8, replace=False)
per hypothesis.  The threshold is 0.003 rad (1.4 px at the first camera's focal length).

tol(case): the bound on |E_all[h] - E_fp64[h]|_F, C_TOL * 2^-24 * sigma_1 / sigma_8 of the sample's A.  The ratio is
what an error of the float rays (2^-24 relative) is amplified by in the null vector.  C_TOL = 4 * the largest
|E(fp64 rays) - E(rays rounded to float)|_F / (2^-24 sigma_1 / sigma_8) over CASES, measured with the fp64
restatement alone (measure_c(); 0.14 on these cases, so C_TOL = 0.56); the 4 is for rays that differ by a last bit
or two between libm implementations.
"""
import functools

import numpy as np

from deftri import matching
from deftri.mapmodel import mat_from_quat
import triangulation_scene as ts

EPI_TH = 0.003
C_TOL = 0.56
# (n, H, seed, nans)
CASES = [(64, 16, 1, 0), (257, 65, 2, 0), (257, 256, 2, 0), (257, 256, 4, 0), (257, 65, 2, 3), (64, 16, 1, 3)]
GPU_SHAPES = [(8, 1, 0), (64, 16, 1), (257, 65, 2), (257, 256, 2)]


def samples(n, H, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(n, 8, replace=False) for _ in range(H)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(n, H, seed, nans=0):
    """A dict: uv1, uv2, k1, k2, T1w, T2w, samples, r1 / r2 (fp64 unit rays), ref64 (find_essential_ransac_ref in fp64),
    cond [H] (sigma_1 / sigma_8 of each sample's A; inf for a sample through a NaN ray).  Shared, not to be modified."""
    uv1, uv2, k1, k2, T1w, T2w, _ = ts.scene(n, nans=nans, seed=seed)
    smp = samples(n, H, seed)
    r1, r2 = matching.unit_rays(k1, uv1), matching.unit_rays(k2, uv2)
    ref64 = matching.find_essential_ransac_ref(r1, r2, smp, EPI_TH)
    with np.errstate(invalid="ignore"):
        cond = np.array([matching.sample_condition(r1[s], r2[s]) if np.isfinite(r1[s]).all() else np.inf for s in smp])
    for a in (uv1, uv2, smp, r1, r2, cond):
        a.setflags(write=False)
    return {"n": n, "H": H, "uv1": uv1, "uv2": uv2, "k1": k1, "k2": k2, "T1w": T1w, "T2w": T2w, "samples": smp, "r1": r1,
            "r2": r2, "ref64": ref64, "cond": cond}


def write_scene(path, key):
    """A case as a raw file for tools/essential_asan.cpp: int32 n, H; float32 threshold, uv1 [2n], uv2 [2n], kb8_1 [8],
    kb8_2 [8]; int32 samples [8H]."""
    c = case(*key)
    with open(path, "wb") as f:
        f.write(np.array([c["n"], c["H"]], np.int32).tobytes())
        for a in (np.float32(EPI_TH), c["uv1"], c["uv2"], c["k1"], c["k2"]):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        f.write(np.ascontiguousarray(c["samples"], np.int32).tobytes())


def tol(c):
    return C_TOL * 2.0 ** -24 * c["cond"]


def measure_c(cases=CASES):
    """The largest |E(fp64 rays) - E(float-rounded rays)|_F / (2^-24 sigma_1 / sigma_8) over the cases' samples."""
    worst = 0.0
    for key in cases:
        c = case(*key)
        f1, f2 = c["r1"].astype(np.float32).astype(np.float64), c["r2"].astype(np.float32).astype(np.float64)
        for h, s in enumerate(c["samples"]):
            if c["ref64"]["degenerate"][h]:
                continue
            Ef = matching.compute_essential(f1[s], f2[s])
            worst = max(worst, float(np.linalg.norm(Ef - c["ref64"]["E_all"][h]) / (2.0 ** -24 * c["cond"][h])))
    return worst


def near_threshold(E_all, c, rel=1e-3):
    """Per hypothesis, the matches whose fp64 error under E_all[h] lies within rel of the threshold (the margins_ok
    convention of triangulation_scene): int [H]."""
    ref = matching.find_essential_ransac_ref(c["r1"], c["r2"], c["samples"], EPI_TH, np.float64, E_all=E_all)
    with np.errstate(invalid="ignore"):
        return (np.abs(ref["err_all"] - EPI_TH) <= rel * EPI_TH).sum(1)


def true_relative_pose(c):
    """(R21, t21) with x2 = R21 x1 + t21, fp64."""
    R1, t1 = c["T1w"].R.astype(np.float64), c["T1w"].t.astype(np.float64)
    R2, t2 = c["T2w"].R.astype(np.float64), c["T2w"].t.astype(np.float64)
    R21 = R2 @ R1.T
    return R21, t2 - R21 @ t1


def noise_free_rays(n, seed):
    """Unit rays of n points seen from a known pose pair without noise, and (R21, t21) with x2 = R21 x1 + t21: fp64,
    R21 orthonormal to fp64 (a float pose's rotation is orthonormal to 3e-8 only)."""
    rng = np.random.default_rng(seed)
    q = np.array([-0.010, 0.015, 0.002, 1.0])
    R21 = mat_from_quat(q / np.linalg.norm(q)).astype(np.float64)
    t21 = np.array([-0.07, -0.005, 0.04])
    x1 = np.stack([rng.uniform(-0.08, 0.08, n), rng.uniform(-0.08, 0.08, n), rng.uniform(0.18, 0.35, n)], 1)
    x2 = x1 @ R21.T + t21
    return x1 / np.linalg.norm(x1, axis=1, keepdims=True), x2 / np.linalg.norm(x2, axis=1, keepdims=True), R21, t21


def _first_best(scores):
    """The reference's rule (:167): replaced on score > bestScore from 0, so the first of the highest, or -1."""
    return int(np.argmax(scores)) if scores.max() > 0 else -1


def check_ransac(ctx, c, round_trips):
    """Context.find_essential_ransac on case c against the restatements; returns the result.
      degenerate flags equal the fp64 restatement's; |E_all[h] - E_fp64[h]|_F <= tol_h;
      scores equal the float32 restatement's under the context's own E_all[h] for every hypothesis none of whose
      fp64 errors lies within rel 1e-3 of the threshold, differ by at most the number of such matches for the others,
      and at most one eighth of the hypotheses are of the second kind;
      best is the first of the highest scores, E_best is E_all[best] bit for bit, inlier.sum() is its score, err lies
      within 2e-6 of the fp64 error under E_best (the bound of the epipolar test)."""
    H, ref = c["H"], c["ref64"]
    r = ctx.find_essential_ransac(c["uv1"], c["uv2"], c["k1"], c["k2"], c["samples"], EPI_TH)
    np.testing.assert_array_equal(r.degenerate, ref["degenerate"])
    assert r.report["n_degenerate"] == int(ref["degenerate"].sum()) and r.report["round_trips"] == round_trips
    assert r.report["n_matches"] == c["n"] and r.report["n_hypotheses"] == H
    ok = ~ref["degenerate"]
    dE = np.linalg.norm((r.E_all.astype(np.float64) - ref["E_all"]).reshape(H, 9), axis=1)
    print(c["n"], H, "max |dE|", dE.max(), "max |dE| / tol", (dE[ok] / tol(c)[ok]).max(initial=0.0))
    assert (dE[ok] <= tol(c)[ok]).all() and not r.E_all[~ok].any() and not r.scores[~ok].any()
    near = near_threshold(r.E_all, c)
    r32 = matching.find_essential_ransac_ref(matching.unit_rays(c["k1"], c["uv1"], np.float32),
                                             matching.unit_rays(c["k2"], c["uv2"], np.float32), c["samples"], EPI_TH, np.float32,
                                             E_all=r.E_all)
    diff = np.abs(r.scores.astype(np.int64) - r32["scores"])
    print("  hypotheses with an error within 1e-3 of the threshold:", int((near > 0).sum()), "of", H, "max |dscore|", diff.max())
    assert (near > 0).mean() <= 0.125
    assert (diff[near == 0] == 0).all() and (diff <= near).all()
    best = _first_best(r.scores)
    assert r.report["best"] == best and r.report["best_score"] == (r.scores[best] if best >= 0 else 0) == int(r.inlier.sum())
    if best < 0:
        assert not r.E.any() and np.isnan(r.err).all()
        return r
    np.testing.assert_array_equal(r.E.view(np.uint32), r.E_all[best].view(np.uint32))
    err64 = matching.epipolar_errors(r.E.astype(np.float64), c["r1"], c["r2"])
    assert np.array_equal(np.isnan(r.err), np.isnan(err64)) and np.nanmax(np.abs(r.err - err64)) <= 2e-6
    with np.errstate(invalid="ignore"):
        far = np.abs(err64 - EPI_TH) > 1e-3 * EPI_TH
        np.testing.assert_array_equal(r.inlier[far], (err64 < EPI_TH)[far])
    return r


def check_cameras(ctx, c, r):
    """Context.reconstruct_cameras of r's best model and inliers against the fp64 restatement from the same E: Rgood
    and t within 1e-5, away equal; the restatement ends at the same t from either starting sign.  Returns (pose,
    away)."""
    pose, away = ctx.reconstruct_cameras(c["uv1"], c["uv2"], c["k1"], c["k2"], r.E, r.inlier)
    Rg, t, aw = matching.reconstruct_cameras_ref(r.E, c["r1"], c["r2"], r.inlier)
    Rg2, t2, aw2 = matching.reconstruct_cameras_ref(r.E, c["r1"], c["r2"], r.inlier, flip_t0=True)
    assert np.array_equal(Rg, Rg2) and np.array_equal(t, t2), "the open sign of U.col(2) decides t on this scene"
    print(c["n"], c["H"], "away", away, aw, aw2, "max |dR|", np.abs(pose.R - Rg).max(), "max |dt|", np.abs(pose.t - t).max())
    assert np.abs(pose.R - Rg).max() <= 1e-5 and np.abs(pose.t - t).max() <= 1e-5 and away == aw
    return pose, away
