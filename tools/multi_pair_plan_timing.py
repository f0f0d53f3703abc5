"""Plan-build times of a multi-keyframe upload: sim.multi_view_problem(N, K) (the C3 / C4 graphs: all pairs of K
keyframes of N correspondences) uploaded three times on one context — cold, then twice more with the plan cache off
(DEFTRI_NO_PLAN_CACHE=1, set here), so every upload builds its plan.  The library's "[deftri upload] plan" lines
(DEFTRI_UPLOAD_TIMING=1, set here) are read back from stderr and printed as one JSON line; with DEFTRI_PLAN_TIMING=1
the per-stage lines pass through to stderr and are counted per name as well.

MULTI_PAIR_BUILDER (deftri_set_multi_pair_builder, with plan builder 1): 0 the plan on the host (default), 1 the device
stages of a multi-pair plan.  LAYOUT_BUILDER (deftri_set_layout_builder): 1 the wave layout on the device too.
MULTI_TILE_BUILDER (deftri_set_multi_tile_builder): 1 the tile layout (build_tiles_multi) on the device too.
An older library under DEFTRI_LIB has no such entries: they are called only when asked for.

usage: python tools/multi_pair_plan_timing.py N K [MULTI_PAIR_BUILDER] [LAYOUT_BUILDER] [MULTI_TILE_BUILDER]"""
import json
import os
import pathlib
import re
import sys
import tempfile
import time

os.environ.setdefault("DEFTRI_UPLOAD_TIMING", "1")
os.environ["DEFTRI_NO_PLAN_CACHE"] = "1"
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "triangulation-in-deformable-scenes_amd"))
from deftri import capi, sim  # noqa: E402

n, k = int(sys.argv[1]), int(sys.argv[2])
multi_pair_builder = int(sys.argv[3]) if len(sys.argv) > 3 else 0
layout_builder = int(sys.argv[4]) if len(sys.argv) > 4 else 0
multi_tile_builder = int(sys.argv[5]) if len(sys.argv) > 5 else 0
p = sim.multi_view_problem(n, k)


def captured(fn):
    """fn() with the process's stderr (the library's lines) kept in a file; returns (seconds, the text)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            t = time.perf_counter()
            fn()
            dt = time.perf_counter() - t
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    sys.stderr.write(text)
    return dt, text


uploads = []
with capi.Context(0) as c:
    c.set_plan("auto")
    c.set_linear_solver("pcg")
    if multi_pair_builder:
        c.set_plan_builder(1)
        c.set_multi_pair_builder(multi_pair_builder)
    if layout_builder:
        c.set_layout_builder(layout_builder)
    if multi_tile_builder:
        c.set_multi_tile_builder(multi_tile_builder)
    for i in range(3):
        dt, text = captured(lambda: c.upload(p))
        m = re.search(r"\[deftri upload\] plan ([0-9.]+) ms, values \+ allocations \+ copies ([0-9.]+) ms", text)
        stages = {}
        for name, ms in re.findall(r"\[deftri plan\] (.+?)\s+([0-9.]+) ms", text):
            stages[name] = round(stages.get(name, 0.0) + float(ms), 2)
        u = {"upload_ms": round(1e3 * dt, 1), "plan_ms": float(m.group(1)) if m else None,
             "rest_ms": float(m.group(2)) if m else None, "stages": stages}
        a = re.search(r"\[deftri plan\] arena ([0-9.]+) MiB of ([0-9.]+), pinned staging ([0-9.]+) MiB", text)
        if a:
            u["arena_mib"], u["arena_reserved_mib"], u["pinned_mib"] = (float(v) for v in a.groups())
        if hasattr(c.lib, "deftri_plan_build_info"):
            u["build_info"] = c.plan_build_info()
        uploads.append(u)
    info = c.plan_info()
out = {"n": n, "k": k, "points": p.n_points, "pairs": p.n_pairs, "arap_edges": int(len(p.arap_pair)),
       "multi_pair_builder": multi_pair_builder, "layout_builder": layout_builder, "multi_tile_builder": multi_tile_builder,
       "plan": info.get("plan"),
       "tiles": info.get("tiles"), "lib": os.environ.get("DEFTRI_LIB", "built"), "cold": uploads[0], "repeated": uploads[1:]}
print(json.dumps(out), flush=True)
