"""Time deftri_find_essential_ransac on the device against the sequential host loops of the same build (a
host-only context), at FeatureExtractor.nFeatures = 2000 matches of tests/triangulation_scene.py and n_hyp = 16 (the
reference's computeMaxTries(0.8, 0.95)), 1024 and 4096 hypotheses drawn by mapping.ransac_samples.

Per n_hyp: one warm-up call per context (it also compares the two), then device and host calls alternating, --reps of
each (the host at most --host-reps: its loop is n_hyp x n evaluations long); the median and the spread (min, max) of
the wall clock per call, which on the device ends in the call's one blocking download, and the device call's
stage times from its report (device events).  Writes profiles/essential_ransac_time.json.

    python tools/essential_time.py [--reps 30] [--host-reps 10] [--out profiles/essential_ransac_time.json]
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (ROOT / "triangulation-in-deformable-scenes_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
from deftri import capi, mapping                           # noqa: E402
import triangulation_scene as ts                           # noqa: E402

N_MATCHES = 2000
HYPOTHESES = (16, 1024, 4096)
EPI_TH = 0.003


def timed(ctx, a):
    t = time.perf_counter()
    r = ctx.find_essential_ransac(*a)
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "essential_ransac_time.json"))
    o = ap.parse_args()
    uv1, uv2, k1, k2, *_ = ts.scene(N_MATCHES, nans=0, seed=0)
    host, dev = capi.Context(-1), capi.Context(0)
    stat = lambda t: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "calls": len(t)}
    res = {"n_matches": N_MATCHES, "epipolar_th": EPI_TH, "reps": o.reps, "host_reps": o.host_reps, "runs": []}
    for H in HYPOTHESES:
        a = (uv1, uv2, k1, k2, mapping.ransac_samples(uv1, H, 10), EPI_TH)
        want, got = host.find_essential_ransac(*a), dev.find_essential_ransac(*a)
        same = (got.E_all.view(np.uint32) == want.E_all.view(np.uint32)).all((1, 2))
        t_dev, t_host, stages = [], [], []
        for k in range(o.reps):
            t, r = timed(dev, a)
            t_dev.append(t)
            stages.append([r.report[s] for s in ("ms_rays", "ms_models", "ms_score")])
            if k < o.host_reps:
                t_host.append(timed(host, a)[0])
        st = np.median(np.array(stages), 0)
        run = {"n_hyp": H, "evaluations": H * N_MATCHES, "models_bit_identical": int(same.sum()),
               "scores_equal": int((got.scores == want.scores).sum()), "best": [got.report["best"], want.report["best"]],
               "best_score": [got.report["best_score"], want.report["best_score"]], "round_trips": got.report["round_trips"],
               "device": dict(stat(t_dev), ms_rays=float(st[0]), ms_models=float(st[1]), ms_score=float(st[2])),
               "host": stat(t_host)}
        run["host_over_device"] = run["host"]["median_ms"] / run["device"]["median_ms"]
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    pathlib.Path(o.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(o.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
