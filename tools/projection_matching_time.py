"""Time deftri_search_with_projection on the device against the sequential host loop of the same build, at the
reference's own size: FeatureExtractor.nFeatures keypoints and as many map points on Data/Realcolon.yaml's grid
(1440 x 1080, 64 x 48 cells, 8 scales of 1.2, nFeatures 2000 as the tests use them).

Every map point has one keypoint with its descriptor near its projection; a fifth of the keypoints have a rival
that an earlier map point may claim, so the claim rounds do real work.  One warm-up call per context (it also
checks that the two agree), then --reps timed calls each; the median and the spread (min, max) of the wall
clock per call, and rounds / round_trips of the device call.  Writes profiles/projection_matching_time.json.

    python tools/projection_matching_time.py [--reps 30] [--out profiles/projection_matching_time.json]
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
from deftri import capi                                    # noqa: E402
import projection_scenes as ps                             # noqa: E402

N_FEATURES = 2000


def time_calls(ctx, a, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = ctx.search_with_projection(*a)
        out.append((time.perf_counter() - t) * 1e3)
    return out, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "projection_matching_time.json"))
    o = ap.parse_args()
    s = ps.timing_scene(N_FEATURES, seed=0)
    a = ps.args(s)
    host, dev = capi.Context(-1), capi.Context(0)
    want, got = host.search_with_projection(*a), dev.search_with_projection(*a)
    agree = all(np.array_equal(getattr(got, k), getattr(want, k)) for k in ("match", "status", "best", "second", "slot_point"))
    t_dev, r = time_calls(dev, a, o.reps)
    t_host, _ = time_calls(host, a, o.reps)
    stat = lambda t: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
    res = {"n_map_points": len(s["pos"]), "n_keypoints": len(s["uv2"]), "reps": o.reps, "device_equals_host": bool(agree),
           "n_matches": r.report["n_matches"], "rounds": r.report["rounds"], "round_trips": r.report["round_trips"],
           "device": dict(stat(t_dev), ms_setup=r.report["ms_setup"], ms_rounds=r.report["ms_rounds"]), "host": stat(t_host)}
    pathlib.Path(o.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(o.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
