"""Time deftri_delaunay2d's star path on the device against the host sweep (delaunay2d) of the same build.

Gaussian clouds of sim.generate_points (the workload's: a dense centre, empty outskirts), float32 coordinates widened
to double, at n = 1,000, 10,000 and 100,000 (the last is C2's keyframe).  The device's triangles are compared with
the sweep's first.  One warm-up call, then `--reps` calls of each by the wall clock in the same process: the device
call is blocking and includes its upload and download; the sweep is timed through its test hook.  Records the marked
stars, the fallback and the report's stage times of the last device call.  Prints one JSON line and writes it to
--out.  There is no pass/fail time.

    python tools/delaunay_time.py [--reps 20] [--out profiles/delaunay_time.json]
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "triangulation-in-deformable-scenes_amd"), str(ROOT / "tests")]

SIZES = (1000, 10000, 100000)


def timed(f, reps):
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        wall.append(1e3 * (time.perf_counter() - t))
    return {"call_ms_median": round(float(np.median(wall)), 4), "call_ms_min": round(min(wall), 4), "call_ms_max": round(max(wall), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "delaunay_time.json"))
    a = ap.parse_args()
    import delaunay_ref as ref
    from deftri import capi

    dev = capi.Context(a.device)
    out = {"reps": a.reps, "points": "sim.generate_points, float32 widened", "sizes": {}}
    for n in SIZES:
        xy = ref.gaussian(n, n)
        want, hull, _ = ref.sweep(xy)
        tris, rep = dev.delaunay(xy)                           # the warm-up, and the check
        assert np.array_equal(tris, want) and rep["hull_size"] == hull
        r = {"n_tris": rep["n_tris"], "hull_size": hull, "path": rep["path"], "fallback": rep["fallback"],
             "marked_stars": rep["host_stars"], "max_degree": rep["max_degree"],
             "host_sweep": timed(lambda: ref.sweep(xy), a.reps), "device_stars": timed(lambda: dev.delaunay(xy), a.reps)}
        rep = dev.delaunay(xy)[1]
        r["device_stage_ms"] = {k: round(rep[k], 4) for k in ("ms_grid", "ms_stars", "ms_host", "ms_total")}
        r["device_over_host"] = round(r["device_stars"]["call_ms_median"] / r["host_sweep"]["call_ms_median"], 4)
        out["sizes"][str(n)] = r
    line = json.dumps(out)
    print(line, flush=True)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(line + "\n")
    dev.close()


if __name__ == "__main__":
    main()
