"""Time deftri_arap_deform and deftri_arap_open3d_optimization on the C2 mesh (100,000 vertices: keyframe 1 of
sim.simulate_two_view's scaled, compacted scene, triangulated by deftri_delaunay2d).

  four_handles   the vertices extreme in x + y and x - y moved up and down in z by a tenth of the scene's z
                 extent, 50 iterations, Spokes: the report's times, the CG iterations of the first and the last
                 global step (runs of 1, 49 and 50 iterations), the time of one CG iteration (first step)
  reference_call arapOpen3DOptimization on the map itself: 500 iterations, one constraint
  splu_baseline  scipy.sparse.linalg.splu of the same system matrix on this host: the factorization and 150 solves
                 (50 global steps of three columns), tests/arap_deform_ref.py's global steps alone

One warm-up call of each device entry first.  Prints one JSON line and writes it to --out.  There is no pass/fail time.

    python tools/arap_deform_time.py [--n 100000] [--device 0] [--out profiles/arap_deform_c2.json]
"""
import argparse
import copy
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "triangulation-in-deformable-scenes_amd"), str(ROOT), str(ROOT / "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "arap_deform_c2.json"))
    a = ap.parse_args()
    from deftri import capi, sim
    import arap_deform_ref as ref

    m, _ = sim.simulate_two_view(n=a.n, seed=1, scale_scene=True, compact=True)
    order = m.kf_order()
    v = np.array([mp.position for mp in m.keyframes[order[1]].map_points if mp is not None], np.float64)
    ctx = capi.Context(a.device)
    tris, drep = ctx.delaunay(v[:, :2])
    s, d = v[:, 0] + v[:, 1], v[:, 0] - v[:, 1]
    ids = np.array([np.argmax(s), np.argmin(s), np.argmax(d), np.argmin(d)], np.int32)
    lift = 0.1 * float(np.ptp(v[:, 2]))
    pos = v[ids].copy()
    pos[:, 2] += lift * np.array([1.0, -1.0, 1.0, -1.0])
    out = {"n": len(v), "n_tris": len(tris), "device": a.device, "handle_lift_m": lift}

    def run(iters):
        t = time.perf_counter()
        _, en, rep = ctx.arap_deform(v, tris, ids, pos, max_iter=iters)
        rep["wall_ms"] = 1e3 * (time.perf_counter() - t)
        return en, rep

    run(1)                                                      # warm-up
    _, r1 = run(1)
    _, r49 = run(a.iters - 1)
    en, r50 = run(a.iters)
    keys = ("iterations", "n_constraints", "n_free", "zero_weight_edges", "cg_iterations", "cg_max_in_step", "on_device",
            "ms_total", "ms_local", "ms_global", "wall_ms", "energy_first", "energy_last", "area")
    out["four_handles"] = {
        **{k: r50[k] for k in keys},
        "cg_iterations_first_step": r1["cg_iterations"], "cg_max_first_step": r1["cg_max_in_step"],
        "cg_iterations_last_step": r50["cg_iterations"] - r49["cg_iterations"],
        "first_step_ms_global": r1["ms_global"],
        "us_per_cg_iteration_first_step": 1e3 * r1["ms_global"] / max(r1["cg_max_in_step"], 1),
        "energies_non_increasing": bool(np.all(np.diff(en) <= 0.0)),
    }
    mm = copy.deepcopy(m)
    ctx.arap_open3d_optimization(copy.deepcopy(m))              # warm-up
    t = time.perf_counter()
    rr = ctx.arap_open3d_optimization(mm)
    out["reference_call"] = {**{k: rr[k] for k in keys if k != "wall_ms"}, "wall_ms": 1e3 * (time.perf_counter() - t),
                             "call_ms": 1e3 * ctx.last_call_s}
    if not a.skip_baseline:
        from scipy.sparse.linalg import splu
        I, J, W, _, _ = ref.edges(v, tris)
        L, free, _ = ref.system_matrix(len(v), I, J, W, ref.constraints(ids, pos))
        t = time.perf_counter()
        lu = splu(L)
        t_fac = time.perf_counter() - t
        b = np.random.default_rng(0).standard_normal((len(v), 3))
        t = time.perf_counter()
        for _ in range(a.iters):
            for c in range(3):
                lu.solve(b[:, c])
        t_sol = time.perf_counter() - t
        out["splu_baseline"] = {"factor_ms": 1e3 * t_fac, "solves": 3 * a.iters, "solves_ms": 1e3 * t_sol,
                                "total_ms": 1e3 * (t_fac + t_sol)}
    line = json.dumps(out)
    print(line, flush=True)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
