"""Time deftri_search_for_triangulation on the device against the host-only context's loop over all pairs, at the
reference's own size: FeatureExtractor.nFeatures = 2000 keypoints in either keyframe (the two-view cloud of
tests/triangulation_matching_scenes.cloud_scene: 1500 planted pairs with noisy descriptors, distractors off the
epipolar line, a tenth of the slots occupied), flag_quirk off so that every row is searched.

One warm-up call per context (it also checks that the two agree), then --reps timed calls each; the median and
the spread (min, max) of the wall clock per call, and the device call's own split.  Writes
profiles/triangulation_matching_time.json.

    python tools/triangulation_matching_time.py [--reps 30] [--commit ID] [--out profiles/triangulation_matching_time.json]
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
import triangulation_matching_scenes as tm                 # noqa: E402

N_FEATURES = 2000


def time_calls(ctx, a, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = ctx.search_for_triangulation(*a)
        out.append((time.perf_counter() - t) * 1e3)
    return out, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "triangulation_matching_time.json"))
    o = ap.parse_args()
    s = tm.cloud_scene(N_FEATURES, N_FEATURES, seed=3, rel=0.0)
    a = tm.args(s, False)
    host, dev = capi.Context(-1), capi.Context(0)
    want, got = host.search_for_triangulation(*a), dev.search_for_triangulation(*a)
    agree = all(np.array_equal(getattr(got, k), getattr(want, k)) for k in ("matches", "best_dist", "status"))
    t_dev, r = time_calls(dev, a, o.reps)
    t_host, _ = time_calls(host, a, o.reps)
    stat = lambda t: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
    res = {"commit": o.commit, "n1": N_FEATURES, "n2": N_FEATURES, "reps": o.reps, "device_equals_host": bool(agree),
           "n_matches": r.n_matches, "n_listed": r.report["n_listed"], "round_trips": r.report["round_trips"],
           "device": dict(stat(t_dev), ms_device=r.report["ms_device"], ms_loop=r.report["ms_loop"]), "host": stat(t_host)}
    pathlib.Path(o.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(o.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
