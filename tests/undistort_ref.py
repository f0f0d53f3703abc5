"""cv::undistortPoints as Frame::undistortKeys and Frame::computeImageBoundaries call it (Frame.cc:221-275),
restated in numpy from its definition (include/deftri.h at deftri_undistort_points) with float64 scalars and one
operation per statement, and Frame::distributeFeatures over it with posInGrid / build_grid of deftri.matching.
Shared by test_undistort.py (host-only context) and test_undistort_gpu.py; it has not been run against an OpenCV
build either.

Also the inputs both files use: the Simulation.yaml calibration, the point set, and the checks of one context
against this reference, so that the device is asked exactly what the host loops are asked."""
import numpy as np

from deftri import matching

F, D = np.float32, np.float64

# Data/Simulation.yaml
CALIB = np.array([458.654, 457.296, 367.215, 248.375], F)
DIST4 = np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05], F)
DIST5 = np.concatenate([DIST4, np.array([0.01], F)])
COLS, ROWS = 752, 480
# the float32 bounds a numpy evaluation of the definition gave for that calibration (the issue's table)
BOUNDS = (-135.79564, -92.875015, 895.5073, 565.5531)
GRID_COLS, GRID_ROWS, N_SCALES, SCALE_FACTOR = 16, 12, 8, 1.2
SIZES = (0, 1, 63, 64, 65, 257)       # one lane, the wave boundary +- 1, a 256-thread block and one lane of the next


def undistort_point(u, v, calib, dist):
    """One point: (float32, float32)."""
    fx, fy, cx, cy = (D(F(c)) for c in calib)
    d = [D(F(c)) for c in dist]
    k1, k2, p1, p2 = d[:4]
    k3 = d[4] if len(d) == 5 else D(0.0)
    one, two = D(1.0), D(2.0)
    with np.errstate(all="ignore"):
        ifx = one / fx
        ify = one / fy
        x0 = D(F(u)) - cx
        x0 = x0 * ifx
        y0 = D(F(v)) - cy
        y0 = y0 * ify
        x, y = x0, y0
        for _ in range(5):
            xx = x * x
            yy = y * y
            r2 = xx + yy
            t = k3 * r2
            t = t + k2
            t = t * r2
            t = t + k1
            t = t * r2
            t = one + t
            icdist = one / t
            if icdist < 0:
                x, y = x0, y0
                break
            a = two * p1                 # dX = 2*p1*x*y + p2*(r2 + 2*x*x)
            a = a * x
            a = a * y
            b = two * x
            b = b * x
            b = r2 + b
            b = p2 * b
            dX = a + b
            a = two * y                  # dY = p1*(r2 + 2*y*y) + 2*p2*x*y
            a = a * y
            a = r2 + a
            a = p1 * a
            b = two * p2
            b = b * x
            b = b * y
            dY = a + b
            x = x0 - dX
            x = x * icdist
            y = y0 - dY
            y = y * icdist
        ou = x * fx
        ou = ou + cx
        ov = y * fy
        ov = ov + cy
        return F(ou), F(ov)


def undistort(uv, calib, dist):
    uv = np.asarray(uv, F).reshape(-1, 2)
    return np.array([undistort_point(u, v, calib, dist) for u, v in uv], F).reshape(-1, 2)


def distort(uv, calib, dist):
    """The forward model (float64): the pixel whose undistortion is about `uv`.  Only builds test inputs."""
    fx, fy, cx, cy = (float(F(c)) for c in calib)
    d = [float(F(c)) for c in dist] + [0.0]
    k1, k2, p1, p2, k3 = d[:5]
    uv = np.asarray(uv, D).reshape(-1, 2)
    x, y = (uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy
    r2 = x * x + y * y
    c = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * c + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * c + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd * fx + cx, yd * fy + cy], 1).astype(F)


def image_bounds(cols, rows, calib, dist):
    """Frame::computeImageBoundaries: float32 [4]."""
    if len(dist) == 0:
        return np.array([0, 0, cols, rows], F)
    o = undistort([[0, 0], [cols, 0], [0, rows], [cols, rows]], calib, dist)
    return np.array([min(o[0, 0], o[2, 0]), min(o[0, 1], o[1, 1]), max(o[1, 0], o[3, 0]), max(o[2, 1], o[3, 1])], F)


def grid_of(bounds, grid_cols=GRID_COLS, grid_rows=GRID_ROWS, n_scales=N_SCALES, scale_factor=SCALE_FACTOR):
    return {"cols": grid_cols, "rows": grid_rows, "min_col": float(bounds[0]), "min_row": float(bounds[1]),
            "max_col": float(bounds[2]), "max_row": float(bounds[3]), "n_scales": n_scales, "scale_factor": float(F(scale_factor))}


def distribute(uv_dis, calib, dist, cols=COLS, rows=ROWS, **grid_args):
    """Frame's bounds, undistortKeys and distributeFeatures: (uv, grid, cell_start, cell_items, in_grid) as
    deftri_distribute_features returns them."""
    uv_dis = np.asarray(uv_dis, F).reshape(-1, 2)
    uv = undistort(uv_dis, calib, dist) if len(dist) else uv_dis.copy()
    grid = grid_of(image_bounds(cols, rows, calib, dist), **grid_args)
    cells = matching.build_grid(grid, uv)
    start, items = [0], []
    for c in range(grid["cols"]):
        for r in range(grid["rows"]):
            items += cells[c][r]
            start.append(len(items))
    in_grid = np.array([matching.pos_in_grid(grid, x, y)[0] for x, y in uv], bool)
    items = np.array(items + [-1] * (len(uv) - len(items)), np.int32)
    return uv, grid, np.array(start, np.int32), items, in_grid


def points():
    """The four corners, the principal point, (cx, 0), and a seeded 257-point uniform sample of the image."""
    rng = np.random.default_rng(20)
    sample = rng.uniform([0, 0], [COLS, ROWS], (257, 2))
    fixed = [[0, 0], [COLS, 0], [0, ROWS], [COLS, ROWS], [CALIB[2], CALIB[3]], [CALIB[2], 0]]
    return np.concatenate([np.array(fixed, D), sample]).astype(F)


# two keypoints of the grid cases, found with this reference and asserted with it in test_undistort.py: under DIST4
# the first undistorts into the last half cell on the right (column index 16 of 16), the second, outside the image,
# to a position that rounds to column -1
LAST_HALF_CELL = (745.0, 10.0)
COLUMN_MINUS_ONE = (-40.0, 240.0)


def grid_keys(n):
    """n keypoint slots for the grid cases: the sample first (so that n = 1 is a lane of its own), from 63 on with
    the two special keypoints, a NaN and a zero slot (a slot behind the extracted keypoints) in front of the end."""
    uv = points()[::-1][:n].copy()
    if n >= 63:
        uv[n - 4] = LAST_HALF_CELL
        uv[n - 3] = COLUMN_MINUS_ONE
        uv[n - 2] = (np.nan, 100.0)
        uv[n - 1] = (0.0, 0.0)
    return uv


def same_bits(got, want):
    """Equal bit for bit; a NaN (whose sign and payload no definition fixes) where the other has one."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape and got.dtype == want.dtype
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def check_points(ctx, uv, calib, dist):
    """undistort_points of `ctx`, also in place, against the reference, bit for bit.  Returns the result."""
    want = undistort(uv, calib, dist)
    got = ctx.undistort_points(uv, calib, dist)
    same_bits(got, want)
    same_bits(ctx.undistort_points(uv, calib, dist, in_place=True), want)
    return got


def check_distribute(ctx, uv_dis, calib, dist, want=None):
    """distribute_features of `ctx` against the reference: every output equal.  Returns the result."""
    w_uv, w_grid, w_start, w_items, w_in = want if want is not None else distribute(uv_dis, calib, dist)
    got = ctx.distribute_features(GRID_COLS, GRID_ROWS, N_SCALES, SCALE_FACTOR, COLS, ROWS, calib, dist, uv_dis)
    same_bits(got.uv, w_uv)
    assert got.grid == w_grid
    np.testing.assert_array_equal(got.cell_start, w_start)
    np.testing.assert_array_equal(got.cell_items, w_items)
    np.testing.assert_array_equal(got.in_grid, w_in)
    return got
