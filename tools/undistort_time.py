"""Time deftri_distribute_features on the device against the sequential host loops of the same build.

The Simulation.yaml calibration (752 x 480, Camera.k1, k2, p1, p2) over a 16 x 12 grid, for frames of nFeatures =
1000 and 5000 slots: four fifths of the slots hold a seeded uniform sample of the image, the rest are the zero slots
behind the extracted keypoints, which undistort to one position and share one cell.  One warm-up call on a device
context, then `--reps` calls by the wall clock (the call is blocking: it ends after its last copy-back), and the
same calls on a host-only context.  The outputs of both contexts are compared first.  Prints one JSON line and
writes it to --out.  There is no pass/fail time.

    python tools/undistort_time.py [--reps 50] [--out profiles/undistort_time.json]
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "triangulation-in-deformable-scenes_amd")]

CALIB = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
DIST = np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05], np.float32)
COLS, ROWS, GRID_COLS, GRID_ROWS, N_SCALES, SCALE_FACTOR = 752, 480, 16, 12, 8, 1.2
SIZES = (1000, 5000)


def slots(n):
    rng = np.random.default_rng(n)
    uv = np.zeros((n, 2), np.float32)
    uv[:4 * n // 5] = rng.uniform([0, 0], [COLS, ROWS], (4 * n // 5, 2))
    return uv


def call(ctx, uv):
    return ctx.distribute_features(GRID_COLS, GRID_ROWS, N_SCALES, SCALE_FACTOR, COLS, ROWS, CALIB, DIST, uv)


def timed(ctx, uv, reps):
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        call(ctx, uv)
        wall.append(1e3 * (time.perf_counter() - t))
    return {"call_ms_median": round(float(np.median(wall)), 4), "call_ms_min": round(min(wall), 4), "call_ms_max": round(max(wall), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "undistort_time.json"))
    a = ap.parse_args()
    from deftri import capi

    dev, host = capi.Context(a.device), capi.Context(-1)
    out = {"image": [COLS, ROWS], "grid": [GRID_COLS, GRID_ROWS], "n_dist": len(DIST), "reps": a.reps, "sizes": {}}
    for n in SIZES:
        uv = slots(n)
        want, got = call(host, uv), call(dev, uv)              # the warm-up, and the check
        for k in ("uv", "cell_start", "cell_items", "in_grid"):
            assert getattr(got, k).tobytes() == getattr(want, k).tobytes(), k
        assert got.grid == want.grid
        r = {"n_in_grid": int(got.cell_start[-1]), "largest_cell": int(np.diff(got.cell_start).max()),
             "device": timed(dev, uv, a.reps), "host_loops": timed(host, uv, a.reps)}
        r["device_over_host"] = round(r["device"]["call_ms_median"] / r["host_loops"]["call_ms_median"], 4)
        out["sizes"][str(n)] = r
    line = json.dumps(out)
    print(line, flush=True)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(line + "\n")
    dev.close(); host.close()


if __name__ == "__main__":
    main()
