"""Time deftri_fast_extract on the device against the sequential host loops of the same build.

Realcolon's shape: a 1440 x 1080 image (a generated scene, tests/features_ref.make_scene at 360 x 270 tiled
4 x 4), 2 scales at 1.66666666, n_max_features 4096, max_keys 2048.  One warm-up call on a device context,
then `--reps` calls by the wall clock (the call is blocking: it ends after its last copy-back), and the same
calls on a host-only context.  Per call the report gives the stage split: the resize and cell kernels between
device events (host clock on the host-only context), the octree on the host, the keypoint stage (mask reads,
orientation, assembly) by the host clock; `other` is the rest of the call (the plan, the allocation, the
copies and the candidates' sort).  The outputs of both contexts are compared first.  Prints one JSON line and
writes it to --out.  There is no pass/fail time.

    python tools/fast_extract_time.py [--reps 20] [--out profiles/fast_extract_time.json]
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "triangulation-in-deformable-scenes_amd"), str(ROOT / "tests")]

PARAMS = dict(n_scales=2, scale_factor=1.66666666, n_max_features=4096, th_fast=10, min_th_fast=4, max_keys=2048)
STAGES = ("ms_resize", "ms_cells", "ms_octree", "ms_keypoints", "ms_total")


def timed(ctx, image, reps):
    wall, stages = [], {k: [] for k in STAGES}
    for _ in range(reps):
        t = time.perf_counter()
        r = ctx.fast_extract(image, PARAMS)
        wall.append(1e3 * (time.perf_counter() - t))
        for k in STAGES:
            stages[k].append(r.report[k])
    med = {k: float(np.median(v)) for k, v in stages.items()}
    med["ms_other"] = med["ms_total"] - sum(med[k] for k in STAGES[:-1])
    return {"call_ms_median": round(float(np.median(wall)), 3), "call_ms_min": round(min(wall), 3), "call_ms_max": round(max(wall), 3),
            "stage_ms_median": {k: round(v, 3) for k, v in med.items()}, "round_trips": r.report["round_trips"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fast_extract_time.json"))
    a = ap.parse_args()
    import features_ref as fr
    from deftri import capi

    image = np.ascontiguousarray(np.tile(fr.make_scene(270, 360, 3)[0], (4, 4)))
    assert image.shape == (1080, 1440)
    dev, host = capi.Context(a.device), capi.Context(-1)
    want = host.fast_extract(image, PARAMS)
    got = dev.fast_extract(image, PARAMS)                      # the warm-up, and the check
    for k in ("uv", "octave", "angle", "response", "size"):
        assert getattr(got, k).tobytes() == getattr(want, k).tobytes(), k
    rep = got.report
    out = {"image": [1440, 1080], "params": PARAMS, "reps": a.reps, "n_keys": rep["n_keys"], "n_candidates": rep["n_candidates"],
           "n_octree": rep["n_octree"], "n_after_mask": rep["n_after_mask"], "device": timed(dev, image, a.reps),
           "host_loops": timed(host, image, a.reps)}
    out["device_over_host"] = round(out["device"]["call_ms_median"] / out["host_loops"]["call_ms_median"], 4)
    line = json.dumps(out)
    print(line, flush=True)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(line + "\n")
    dev.close(); host.close()


if __name__ == "__main__":
    main()
