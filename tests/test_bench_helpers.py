"""bench.py's host-side helpers on CPU: --steps is the number of timed steps whatever the LM does
(timed_steps), and --dump-outputs writes float64 .npy files within its byte budget (dump_outputs)."""
import numpy as np


def _report(iterations, chi0, chi1):
    return {"iterations": iterations, "trials_total": 2 * iterations, "pcg_iterations": 5 * iterations,
            "ms_total": 1.0, "ms_factor": -1.0, "chi2_initial": chi0, "chi2_final": chi1, "lambda_final": 7.0,
            "chi2_iter": [chi1] * iterations}


def test_timed_steps_single_solve():
    import bench
    calls, resets = [], []
    rep, solves = bench.timed_steps(lambda k: calls.append(k) or _report(k, 10.0, 1.0), lambda: resets.append(1), 20)
    assert calls == [20] and resets == [] and solves == 1
    assert rep == _report(20, 10.0, 1.0)


def test_timed_steps_restarts_after_early_stop():
    import bench
    calls, resets = [], []

    def solve(k):                         # an LM that terminates after 8 iterations at the most
        calls.append(k)
        return _report(min(k, 8), 10.0, 3.0 + len(calls))

    rep, solves = bench.timed_steps(solve, lambda: resets.append(1), 20)
    assert calls == [20, 12, 4] and len(resets) == 2 and solves == 3
    assert rep["iterations"] == 20 and rep["trials_total"] == 40 and rep["pcg_iterations"] == 100
    assert rep["ms_total"] == 3.0 and rep["ms_factor"] == -1.0
    assert rep["chi2_initial"] == 10.0 and rep["chi2_final"] == 6.0 and len(rep["chi2_iter"]) == 4


def test_timed_steps_gives_up_on_empty_solve():
    import bench
    n = []
    rep, solves = bench.timed_steps(lambda k: n.append(k) or _report(3 if len(n) == 1 else 0, 1.0, 1.0), lambda: None, 5)
    assert n == [5, 2] and solves == 1 and rep["iterations"] == 3


def test_dump_outputs_whole(tmp_path):
    import bench
    pts = np.arange(30, dtype=np.float64).reshape(10, 3)
    bench.dump_outputs(tmp_path / "out", {"points": pts, "chi2": [2.0, 1.0], "chi2_iter": []})
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["chi2.npy", "chi2_iter.npy", "points.npy"]
    got = np.load(tmp_path / "out" / "points.npy")
    assert got.dtype == np.float64 and np.array_equal(got, pts)
    assert np.load(tmp_path / "out" / "chi2_iter.npy").shape == (0,)


def test_dump_outputs_samples_over_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 3 << 20)
    pts = np.arange(3 * 200000, dtype=np.float64).reshape(200000, 3)        # 4.8 MB
    small = np.ones((4, 7))
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"points": pts, "pair_transforms": small})
    a, rows = np.load(tmp_path / "a" / "points.npy"), np.load(tmp_path / "a" / "points_rows.npy")
    assert a.dtype == np.float64 and rows.dtype == np.float64
    assert 0 < len(a) < len(pts) and len(rows) == len(a) and np.all(np.diff(rows) > 0)
    assert np.array_equal(a, pts[rows.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "a" / "pair_transforms.npy"), small)
    assert a.nbytes + rows.nbytes + small.nbytes <= 3 << 20                  # the budget counts payload bytes
    assert np.array_equal(rows, np.load(tmp_path / "b" / "points_rows.npy"))     # the sample is fixed
