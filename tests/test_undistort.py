"""deftri_undistort_points, deftri_image_bounds and deftri_distribute_features on a host-only context (the
sequential loops of csrc/undistort.hip) against undistort_ref.py, the numpy restatement of cv::undistortPoints'
definition and of Frame::computeImageBoundaries / undistortKeys / distributeFeatures (Frame.cc:188-275), and the
Python layer over them (Settings.distortion, matching.frame_grid, features.distribute).

The library and the reference evaluate the same double operations in the same order with one rounding each, so
every float is compared bit for bit; the cell lists are integers.  No GPU: test_undistort_gpu.py asks the device
the same questions."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN
from deftri import capi, features, matching
from deftri.settings import Settings
import undistort_ref as ur

F = np.float32


@pytest.fixture(scope="module")
def host():
    ctx = capi.Context(-1)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def sim_settings():
    return Settings(path=GOLDEN / "sim_default" / "settings.yaml")


@pytest.mark.parametrize("dist", [ur.DIST4, ur.DIST5], ids=["k1k2p1p2", "k3"])
def test_points(host, dist):
    uv = ur.points()
    got = ur.check_points(host, uv, ur.CALIB, dist)
    assert np.abs(got - uv).max() > 1.0 and np.isfinite(got).all()          # the distortion is not a no-op here
    assert got[4].tolist() == [ur.CALIB[2], ur.CALIB[3]]                       # the principal point stays
    assert host.undistort_points(uv[:0], ur.CALIB, dist).shape == (0, 2)      # n = 0


def test_k3_changes_the_result(host):
    uv = ur.points()
    assert (host.undistort_points(uv, ur.CALIB, ur.DIST4) != host.undistort_points(uv, ur.CALIB, ur.DIST5)).any()


def test_negative_icdist(host):
    """k1 = -2 at normalized radius 1: icdist = 1 / (1 - 2) < 0 in the first iteration, the point is given up and the
    output is the round trip of the distorted position."""
    dist = np.array([-2, 0, 0, 0], F)
    u = F(F(ur.CALIB[2]) + F(ur.CALIB[0]))
    uv = np.array([[u, ur.CALIB[3]], [ur.CALIB[2], F(ur.CALIB[3] - ur.CALIB[1])], [400.0, 250.0]], F)
    got = ur.check_points(host, uv, ur.CALIB, dist)
    fx, cx = np.float64(ur.CALIB[0]), np.float64(ur.CALIB[2])
    x0 = (np.float64(u) - cx) * (np.float64(1) / fx)
    assert 1 / (1 - 2 * x0 * x0) < 0 and got[0, 0] == F(x0 * fx + cx)
    assert np.abs(got[2] - uv[2]).max() > 0.01                                # a point near the centre still iterates


def test_zero_coefficients(host):
    """dist = 0 still runs the path: the output is float(((u - cx) * ifx) * fx + cx), not always u."""
    ur.check_points(host, ur.points(), ur.CALIB, np.zeros(4, F))
    ur.check_points(host, ur.points(), ur.CALIB, np.zeros(5, F))


def test_nan_input(host):
    uv = np.array([[np.nan, 100.0], [100.0, np.nan], [300.0, 200.0]], F)
    got = ur.check_points(host, uv, ur.CALIB, ur.DIST4)
    assert np.isnan(got[0, 0]) and np.isnan(got[1, 1]) and np.isfinite(got[2]).all()
    res = ur.check_distribute(host, uv, ur.CALIB, ur.DIST4)
    assert res.in_grid.tolist() == [False, False, True] and res.cell_items.tolist() == [2, -1, -1]


def test_bounds(host):
    got = host.image_bounds(ur.COLS, ur.ROWS, ur.CALIB, ur.DIST4)
    want = ur.image_bounds(ur.COLS, ur.ROWS, ur.CALIB, ur.DIST4)
    assert got.dtype == F and got.tobytes() == want.tobytes()
    assert np.abs(got.astype(np.float64) - np.array(ur.BOUNDS)).max() < 1e-3
    assert got[0] < 0 and got[1] < 0                                          # the matchers' subtraction is exercised
    assert host.image_bounds(ur.COLS, ur.ROWS).tolist() == [0, 0, 752, 480]
    assert host.image_bounds(ur.COLS, ur.ROWS, ur.CALIB, []).tolist() == [0, 0, 752, 480]
    got5 = host.image_bounds(ur.COLS, ur.ROWS, ur.CALIB, ur.DIST5)
    assert got5.tobytes() == ur.image_bounds(ur.COLS, ur.ROWS, ur.CALIB, ur.DIST5).tobytes() != got.tobytes()


def test_special_keypoints_of_the_grid_cases():
    """What undistort_ref.grid_keys plants, by the reference alone."""
    uv, grid, _, _, in_grid = ur.distribute([ur.LAST_HALF_CELL, ur.COLUMN_MINUS_ONE], ur.CALIB, ur.DIST4)
    w, h = matching._inverses(grid)
    col = [float(F(F(x - F(grid["min_col"])) * w)) for x in uv[:, 0]]
    row = [float(F(F(y - F(grid["min_row"])) * h)) for y in uv[:, 1]]
    assert uv[0, 0] < grid["max_col"] and 15.5 <= col[0] < 16 and -1.5 < col[1] < -0.5     # inside the bounds, yet column 16
    assert all(0 <= round(r) < ur.GRID_ROWS for r in row) and not in_grid.any()


@pytest.mark.parametrize("n", ur.SIZES)
def test_distribute(host, n):
    uv_dis = ur.grid_keys(n)
    res = ur.check_distribute(host, uv_dis, ur.CALIB, ur.DIST4)
    assert res.cells() == matching.build_grid(res.grid, res.uv)
    if n >= 63:
        assert res.in_grid[n - 4:].tolist() == [False, False, False, True]    # half cell, column -1, NaN, a zero slot
        assert not np.isin(np.arange(n - 4, n - 1), res.cell_items).any()
        o = ur.undistort_point(0, 0, ur.CALIB, ur.DIST4)                       # the zero slot is undistorted like any other
        assert res.uv[n - 1].tolist() == [o[0], o[1]] and res.cells()[0][0][-1] == n - 1
        assert 0 < res.cell_start[-1] < n and max(len(c) for col in res.cells() for c in col) >= 2
    # without coefficients: a copy, and the grid over 0, 0, cols, rows
    plain = ur.check_distribute(host, uv_dis, ur.CALIB, [])
    assert (plain.grid["min_col"], plain.grid["min_row"], plain.grid["max_col"], plain.grid["max_row"]) == (0, 0, 752, 480)
    assert plain.cells() == matching.build_grid(plain.grid, uv_dis)
    ur.same_bits(plain.uv, uv_dis)


def test_distribute_five_coefficients(host):
    ur.check_distribute(host, ur.grid_keys(65), ur.CALIB, ur.DIST5)


def test_settings(host, sim_settings):
    text = (GOLDEN / "sim_default" / "settings.yaml").read_text()
    s = sim_settings
    assert s.has_distortion and s.distortion.dtype == F and s.distortion.tobytes() == ur.DIST4.tobytes()
    s5 = Settings(text=text + "\nCamera.k3: 0.01\n")
    assert s5.distortion.tobytes() == ur.DIST5.tobytes()
    plain = Settings(text="\n".join(ln for ln in text.splitlines() if not ln.startswith(("Camera.k", "Camera.p"))))
    assert not plain.has_distortion and plain.distortion.shape == (0,) and plain.distortion.dtype == F
    d = Settings(text="Camera.d1: 0.25\nCamera.k1: -0.5\n")
    assert d.k1 == 0.25 and d.distortion.tolist() == [-0.5, 0, 0, 0]           # settings.k1 is still Camera.d1


def test_frame_grid(host, sim_settings):
    s = Settings(text=(GOLDEN / "sim_default" / "settings.yaml").read_text()
                 + "\nFeatureGrid.nGridCols: 16\nFeatureGrid.nGridRows: 12\nFeatureExtractor.nScales: 8\n"
                   "FeatureExtractor.fScaleFactor: 1.2\n")
    assert (int(s.cols), int(s.rows)) == (ur.COLS, ur.ROWS)
    g = matching.frame_grid(host, s)
    assert g == dict(ur.grid_of(ur.image_bounds(ur.COLS, ur.ROWS, ur.CALIB, ur.DIST4)), scale_factor=1.2)   # the YAML's double, as feature_grid
    assert np.abs(np.array([g["min_col"], g["min_row"], g["max_col"], g["max_row"]]) - np.array(ur.BOUNDS)).max() < 1e-3
    with pytest.raises(ValueError, match="Camera.k1"):
        matching.feature_grid(s)
    plain = Settings(text="Camera.cols: 752\nCamera.rows: 480\nFeatureGrid.nGridCols: 16\nFeatureGrid.nGridRows: 12\n"
                          "FeatureExtractor.nScales: 8\nFeatureExtractor.fScaleFactor: 1.2\n")
    assert matching.frame_grid(host, plain) == matching.feature_grid(plain)
    with pytest.raises(ValueError, match="Camera.k1"):                        # the undistortion would divide by fx
        matching.frame_grid(None, Settings(text="Camera.k1: 0.1\nCamera.fy: 400\n"))
    # features.distribute is distribute_features with the settings' values
    d = features.distribute(host, ur.grid_keys(65), s)
    ur.check_distribute(host, ur.grid_keys(65), ur.CALIB, ur.DIST4)
    assert d.grid == dict(g, scale_factor=float(F(1.2))) and d.cell_items.tolist() == ur.distribute(ur.grid_keys(65), ur.CALIB, ur.DIST4)[3].tolist()
    padded = features.distribute(host, ur.grid_keys(65)[:3], s, n_slots=7)
    assert len(padded) == 7 and (padded.uv[3:] == padded.uv[3]).all() and padded.in_grid[3:].all()


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def test_errors(host):
    """Every DEFTRI_E_ARG case sets a message and leaves the outputs untouched."""
    lib, h = host.lib, host.h
    uv = ur.grid_keys(5); out = np.full_like(uv, 7)
    calib, dist = ur.CALIB.copy(), ur.DIST4.copy()
    g = capi._abi.FeatureGrid()
    start = np.full(ur.GRID_COLS * ur.GRID_ROWS + 1, 7, np.int32); items = np.full(5, 7, np.int32)

    def message(rc, *words):
        msg = (lib.deftri_last_error(h) or b"").decode()
        assert rc == capi._abi.DEFTRI_E_ARG and msg and all(w in msg for w in words), (rc, msg)

    def points(n=5, uv_in=_fp(uv), calib=_fp(calib), dist=_fp(dist), n_dist=4, uv_out=_fp(out)):
        return lib.deftri_undistort_points(h, n, uv_in, calib, dist, n_dist, uv_out)

    def bounds(calib=_fp(calib), dist=_fp(dist), n_dist=4, b=_fp(out)):
        return lib.deftri_image_bounds(h, ur.COLS, ur.ROWS, calib, dist, n_dist, b)

    def distribute(gc=ur.GRID_COLS, gr=ur.GRID_ROWS, ns=8, calib=_fp(calib), dist=_fp(dist), n_dist=4, n=5, uv_dis=_fp(uv), uv_out=_fp(out),
                   grid=C.byref(g), cs=_ip(start), ci=_ip(items), cols=ur.COLS):
        return lib.deftri_distribute_features(h, gc, gr, ns, 1.2, cols, ur.ROWS, calib, dist, n_dist, n, uv_dis, uv_out, grid, cs, ci, None)

    assert points() == 0 and bounds() == 0 and distribute() == 0               # the defaults are a valid call
    out[:] = 7; start[:] = 7; items[:] = 7
    for kw in ({"uv_in": None}, {"uv_out": None}, {"calib": None}, {"dist": None}):
        message(points(**kw), "undistort_points", "null")
    message(points(n=-1), "undistort_points", "negative")
    for nd in (0, 3, 6):
        message(points(n_dist=nd), "undistort_points", "n_dist")
    message(bounds(b=None), "image_bounds", "null")
    message(bounds(calib=None), "image_bounds", "null")
    message(bounds(n_dist=3), "image_bounds", "n_dist")
    for kw in ({"uv_dis": None}, {"uv_out": None}, {"grid": None}, {"cs": None}, {"ci": None}, {"calib": None}, {"dist": None}):
        message(distribute(**kw), "distribute_features", "null")
    message(distribute(n=-1), "distribute_features", "negative")
    message(distribute(n_dist=2), "distribute_features", "n_dist")
    message(distribute(gc=0), "distribute_features", "nGridCols")
    message(distribute(gr=-1), "distribute_features", "nGridCols")
    message(distribute(gc=4097, gr=4096), "distribute_features", "2^24")
    message(distribute(ns=0), "distribute_features", "nScales")
    message(distribute(cols=0, n_dist=0), "distribute_features", "max <= min")
    for bad in (0.0, np.inf, np.nan):
        for k in (0, 1):
            c = ur.CALIB.copy(); c[k] = bad
            message(points(calib=_fp(c)), "undistort_points", "Camera.fx")
            message(bounds(calib=_fp(c)), "image_bounds", "Camera.fx")
            message(distribute(calib=_fp(c)), "distribute_features", "Camera.fx")
    # max <= min after undistortion: a principal point that is not a number
    c = ur.CALIB.copy(); c[2] = np.nan
    message(bounds(calib=_fp(c)), "image_bounds", "max <= min")
    message(distribute(calib=_fp(c)), "distribute_features", "max <= min", "after undistortion")
    assert (out == 7).all() and (start == 7).all() and (items == 7).all()
    # fx = 0 without coefficients is no error: nothing divides by it
    c = ur.CALIB.copy(); c[0] = 0
    assert distribute(calib=_fp(c), n_dist=0) == 0 and bounds(calib=_fp(c), n_dist=0) == 0
