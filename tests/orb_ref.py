"""ORB::describe (reference Modules/Features/ORB.cc:20-90, ORB.h:34-68) restated in numpy for the tests of
deftri_orb_describe.  It shares no code with csrc/: the library is held to it exactly.

OpenCV's parts (the 8-bit bilinear resize, copyMakeBorder with BORDER_REFLECT_101, the 8-bit separable
Gaussian the reference's call takes) follow their definitions as include/deftri.h states them; OpenCV itself
is not a test dependency.  The sampling table of the reference is not here either: synthetic_pattern() draws a
seeded one.
"""
import math

import numpy as np

import features_ref as fr

F = np.float32
BORDER = 19                   # EDGE_THRESHOLD


def synthetic_pattern(seed, lim=13):
    """512 integer points uniform in [-lim, lim]^2, int32 [512, 2]; lim = 13 keeps every rotated offset within
    18 pixels (13 * sqrt(2) = 18.4 rounds to 18)."""
    return np.random.default_rng(seed).integers(-lim, lim + 1, size=(512, 2)).astype(np.int32)


def scale_tables(n_scales, scale_factor):
    """ORB.h:39-49."""
    f = F(scale_factor)
    scale = [F(1.0)]
    for _ in range(1, n_scales):
        scale.append(F(scale[-1] * f))
    return scale, [F(F(1.0) / s) for s in scale]


def blur_kernel():
    """getGaussianKernel(7, 2, CV_32F) as the 8-bit separable filter takes it: cvRound(k * 256)."""
    x = np.arange(-3, 4, dtype=np.float64)
    w = np.exp(-(x * x) / 8.0)
    k = (w / w.sum()).astype(F)
    return np.rint(k * F(256)).astype(np.int64)


def reflect101(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def add_border(img, by=BORDER):
    """copyMakeBorder(img, by on every side, BORDER_REFLECT_101)."""
    rows, cols = img.shape
    ys = reflect101(np.arange(-by, rows + by), rows)
    xs = reflect101(np.arange(-by, cols + by), cols)
    return img[np.ix_(ys, xs)]


def blur_u8(img):
    """GaussianBlur(img, Size(7, 7), 2, 2, BORDER_REFLECT_101) on 8-bit data by the generic separable filter:
    integer kernels, plain int sums, (s + 32768) >> 16 saturated."""
    k = blur_kernel()
    rows, cols = img.shape
    p = add_border(img, 3).astype(np.int64)
    row = sum(k[j] * p[:, j:j + cols] for j in range(7))                  # [rows + 6, cols]
    col = sum(k[j] * row[j:j + rows, :] for j in range(7))                # [rows, cols]
    return np.clip((col + 32768) >> 16, 0, 255).astype(np.uint8)


def pyramid(image, inv):
    """ORB::computePyramid (ORB.cc:32-52).  Returns (levels with their border, the unblurred interiors)."""
    rows, cols = image.shape
    levels, plains = [], []
    for l in range(len(inv)):
        r, c = fr.cv_round(F(rows) * inv[l]), fr.cv_round(F(cols) * inv[l])
        if l == 0:
            assert (r, c) == (rows, cols)
            plain = image.copy()
        else:
            above = levels[-1][BORDER:-BORDER, BORDER:-BORDER]            # the blurred interior: the blur is in place
            plain = fr.resize_linear_u8(above, r, c)
        level = add_border(plain).copy()
        level[BORDER:-BORDER, BORDER:-BORDER] = blur_u8(plain)            # the border keeps the unblurred reflections
        levels.append(level)
        plains.append(plain)
    return levels, plains


def rotation(angle_deg):
    """a, b of computeORBDescriptor (:55-56) as float32, through libm's double cos and sin."""
    rad = F(F(angle_deg) * F(math.pi / 180.0))
    if not np.isfinite(rad):
        return F(np.nan), F(np.nan)
    return F(math.cos(float(rad))), F(math.sin(float(rad)))


def sample_positions(uv, octave, angle, inv, pattern):
    """Per keypoint the (row, column) of its 512 samples relative to the level's interior, float32 [512] each,
    rounded but not converted, and the offsets before rounding."""
    a, b = rotation(angle)
    with np.errstate(invalid="ignore", over="ignore"):
        cx = np.rint(F(F(uv[0]) * inv[octave]))
        cy = np.rint(F(F(uv[1]) * inv[octave]))
        px, py = pattern[:, 0].astype(F), pattern[:, 1].astype(F)
        row_raw = (px * b).astype(F) + (py * a).astype(F)
        col_raw = (px * a).astype(F) - (py * b).astype(F)
        return F(cy) + np.rint(row_raw), F(cx) + np.rint(col_raw), row_raw, col_raw


def describe(image, n_scales, scale_factor, uv, octave, angle, pattern):
    """ORB::describe.  Returns a dict: desc uint8 [n, 32], status uint8 [n], levels, plains, and per keypoint
    the sample rows / columns (None where status is 1) and raw offsets."""
    _scale, inv = scale_tables(n_scales, scale_factor)
    levels, plains = pyramid(image, inv)
    pattern = np.asarray(pattern).reshape(512, 2)
    n = len(octave)
    desc = np.zeros((n, 32), np.uint8)
    status = np.zeros(n, np.uint8)
    rows_of, cols_of, raw = [], [], []
    for i in range(n):
        l = int(octave[i])
        lr, lc = plains[l].shape
        r, c, rr, cr = sample_positions(uv[i], l, angle[i], inv, pattern)
        raw.append((rr, cr))
        with np.errstate(invalid="ignore"):
            inside = (r >= -BORDER) & (r < lr + BORDER) & (c >= -BORDER) & (c < lc + BORDER)
        if not inside.all():                                              # NaN compares false: outside
            status[i] = 1
            rows_of.append(None); cols_of.append(None)
            continue
        ri, ci = r.astype(np.int64), c.astype(np.int64)
        rows_of.append(ri); cols_of.append(ci)
        v = levels[l][ri + BORDER, ci + BORDER].astype(np.int64)
        bits = (v[0::2] < v[1::2]).astype(np.uint8)                        # comparison c reads points 2c, 2c + 1
        desc[i] = np.packbits(bits.reshape(32, 8), axis=1, bitorder="little")[:, 0]
    return {"desc": desc, "status": status, "levels": levels, "plains": plains, "rows": rows_of, "cols": cols_of, "raw": raw,
            "inv": inv}
