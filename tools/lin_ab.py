"""Bit identity and speed of the linearization between builds of libdeftri.so on one GPU: each library
in a fresh child process (DEFTRI_LIB), on C2 (two views, N_CORR correspondences) and on the 8-keyframe
all-pairs shape of tests/test_gpu_sp.py (28 pairs, 56 scales).  Per library and shape: b and the
Hessian diagonal at the uploaded state, the chi2 history and the final state of N_IT numeric-Jacobian
LM iterations (compared exactly with the first library's), the profiled trial's linearization kernels
and the best of a few timed solves.

usage: python tools/lin_ab.py OUT.json N_CORR N_IT LIB [LIB ...]"""
import hashlib
import json
import os
import pathlib
import subprocess
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent


def run_one(out_npz, n, n_it):
    sys.path.insert(0, str(ROOT / "triangulation-in-deformable-scenes_amd"))
    import numpy as np
    import torch  # noqa: F401  (the HIP runtime first, as bench.py)
    from deftri import capi, sim
    arrays, res = {}, {}
    mv_map, _ = sim.simulate_multi_view(n=100, k=8, seed=1)
    host = capi.Context(-1)
    mv = host.build_graph(mv_map, 1.0, 1e7, np.float32(0.3))
    host.close()
    for name, p in (("c2", sim.two_view_problem(n, 1)), ("mv8", mv)):
        with capi.Context(0) as ctx:
            ctx.set_plan("iterative")
            ctx.upload(p)
            b, d = ctx.gradient()
            r = ctx.solve_lm(n_it, analytic=False)
            pts, sc, tg = ctx.download()
            b1, d1 = ctx.gradient()
            arrays.update({f"{name}_b": b, f"{name}_diag": d, f"{name}_chi2_iter": np.array(r["chi2_iter"]),
                           f"{name}_points": pts, f"{name}_scales": sc, f"{name}_tg": tg, f"{name}_b_end": b1,
                           f"{name}_diag_end": d1})
            st = ctx.profile_trial(r["lambda_final"])
            lin = {k: round(1e3 * v["ms"], 2) for k, v in st.items() if "glin" in k or k.startswith("lin_") or k == "arap_pre"}
            dts = []
            for _ in range(5):
                ctx.reset_state()
                torch.cuda.synchronize()
                t = time.perf_counter()
                r2 = ctx.solve_lm(25, analytic=False)
                torch.cuda.synchronize()
                dts.append((time.perf_counter() - t) / max(r2["iterations"], 1))
            res[name] = {"lin_us": lin, "lin_us_sum": round(sum(lin.values()), 2), "trials": r["trials_iter"],
                         "ms_per_lm_iteration": [round(1e3 * x, 4) for x in dts]}
    np.savez(out_npz, **arrays)
    res["sha256"] = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] for k, v in arrays.items()}
    return res


if __name__ == "__main__":
    if sys.argv[1] == "--one":
        print("RESULT " + json.dumps(run_one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))), flush=True)
        sys.exit(0)
    import numpy as np
    out, n, n_it, libs = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4:]
    runs, ref = [], None
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(libs):
            npz = os.path.join(tmp, f"{i}.npz")
            res = subprocess.run([sys.executable, __file__, "--one", npz, str(n), str(n_it)],
                                 env=dict(os.environ, DEFTRI_LIB=str(pathlib.Path(lib).resolve())),
                                 capture_output=True, text=True, timeout=900)
            line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
            if res.returncode or not line:
                print(json.dumps({"lib": lib, "rc": res.returncode, "stderr": res.stderr[-3000:]}), flush=True)
                sys.exit(1)
            r = json.loads(line[0][7:])
            r["lib"] = os.path.basename(lib)
            a = dict(np.load(npz))
            if ref is None:
                ref = a
            r["identical_to_first"] = {k: bool(a[k].shape == ref[k].shape and np.array_equal(a[k], ref[k])) for k in ref}
            runs.append(r)
            print(json.dumps(r), flush=True)
    same = all(all(r["identical_to_first"].values()) for r in runs)
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text(json.dumps({"n_corr": n, "lm_iterations": n_it, "all_identical": same, "runs": runs}, indent=1) + "\n")
    print("all identical:", same, flush=True)
    sys.exit(0 if same else 2)
