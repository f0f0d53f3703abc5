"""Stage times of the drop-in arapOptimization call (bench.py's end_to_end: cold, warm, next round) at
N_CORR correspondences: run with DEFTRI_CALL_TIMING=1 DEFTRI_PLAN_TIMING=1 DEFTRI_GRAPH_TIMING=1
DEFTRI_UPLOAD_TIMING=1 to get the library's per-stage lines on stderr.

MESH_BUILDER (deftri_set_mesh_builder): 0 the host sweep (default), 1 the Delaunay stars on the device.
PLAN_BUILDER (deftri_set_plan_builder): 0 the host passes (default), 1 the plan's sorts and scans on the device.
TILE_BUILDER (deftri_set_tile_builder): 0 build_tiles on the host (default), 1 the tile layout on the device too.
LAYOUT_BUILDER (deftri_set_layout_builder): 0 the phase-1 blocks and the wave layout on the host (default), 1 on
the device too, pmap and pidx staying there.
GRAPH_BUILDER (deftri_set_graph_builder): 0 the graph build's passes on the host (default), 1 the device stages.

usage: python tools/e2e_timing.py [N_CORR] [MESH_BUILDER] [PLAN_BUILDER] [TILE_BUILDER] [LAYOUT_BUILDER] [GRAPH_BUILDER]"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "triangulation-in-deformable-scenes_amd"))
import torch  # noqa: F401,E402
import bench  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
mesh_builder = int(sys.argv[2]) if len(sys.argv) > 2 else 0
plan_builder = int(sys.argv[3]) if len(sys.argv) > 3 else 0
tile_builder = int(sys.argv[4]) if len(sys.argv) > 4 else 0
layout_builder = int(sys.argv[5]) if len(sys.argv) > 5 else 0
graph_builder = int(sys.argv[6]) if len(sys.argv) > 6 else 0
p, m = bench.build_problem(n, 1)


def configure(c):
    c.set_plan("auto")
    c.set_mesh_builder(mesh_builder)
    if plan_builder:                       # (an older library under DEFTRI_LIB has no such entry)
        c.set_plan_builder(plan_builder)
    if tile_builder:
        c.set_tile_builder(tile_builder)
    if layout_builder:
        c.set_layout_builder(layout_builder)
    if graph_builder:
        c.set_graph_builder(graph_builder)


out = bench.end_to_end(0, m, configure)
out["mesh_builder"] = mesh_builder
out["plan_builder"] = plan_builder
out["tile_builder"] = tile_builder
out["layout_builder"] = layout_builder
out["graph_builder"] = graph_builder
print(json.dumps(out), flush=True)
