"""Time deftri_match_for_initialization on the device and its sequential host loop.

For each size (2,048 keypoints per frame, Realcolon's FeatureExtractor.nFeatures, and 100,000 per frame,
the C2 size) on Realcolon's grid (64 x 48 cells over 1440 x 1080, radius 25, th 100): one warm-up call,
then `--reps` calls on a device context timed with events around the call (the call copies its inputs in
and its results out, so this is the whole entry), and the same calls on a host-only context by the wall
clock.  Prints one JSON line per size.  There is no pass/fail time.

    python tools/match_timing.py [--sizes 2048 100000] [--reps 5]
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "triangulation-in-deformable-scenes_amd"), str(ROOT)]

GRID = dict(cols=64, rows=48, min_col=0.0, min_row=0.0, max_col=1440.0, max_row=1080.0, n_scales=8, scale_factor=1.2)


def scene(n, seed=0, radius=25.0):
    """n reference keypoints over the image; the current frame is a permutation of them shifted by less than
    the radius, descriptors with about five bits in 256 flipped; a fifth of either frame of a coarser octave."""
    rng = np.random.default_rng(seed)
    uv1 = (rng.uniform(0, 1, (n, 2)) * [1440.0, 1080.0]).astype(np.float32)
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    flips = np.packbits(rng.random((n, 256)) < 0.02, axis=1)
    perm = rng.permutation(n)
    uv2 = np.empty_like(uv1); d2 = np.empty_like(d1)
    uv2[perm] = uv1 + rng.uniform(-0.9 * radius, 0.9 * radius, (n, 2)).astype(np.float32)
    d2[perm] = d1 ^ flips
    o1 = np.where(rng.random(n) < 0.2, 1, 0).astype(np.int32)
    o2 = np.where(rng.random(n) < 0.2, 2, 0).astype(np.int32)
    return (GRID, uv1, o1, d1, uv2, o2, d2, 100, radius)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 100000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    from deftri import capi

    dev = capi.Context(a.device)
    host = capi.Context(-1)
    for n in a.sizes:
        s = scene(n)
        want = host.match_for_initialization(*s)
        got = dev.match_for_initialization(*s)                     # the warm-up, and the check
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3] == want[3]
        dev_ms, host_ms = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dev.match_for_initialization(*s)
            e1.record()
            e1.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
            t = time.perf_counter()
            host.match_for_initialization(*s)
            host_ms.append(1e3 * (time.perf_counter() - t))
        print(json.dumps({"n_per_frame": n, "n_matches": got[3], "device_ms": [round(x, 3) for x in dev_ms],
                          "host_loop_ms": [round(x, 3) for x in host_ms], "device_ms_median": round(float(np.median(dev_ms)), 3),
                          "host_loop_ms_median": round(float(np.median(host_ms)), 3)}), flush=True)
    dev.close(); host.close()


if __name__ == "__main__":
    main()
