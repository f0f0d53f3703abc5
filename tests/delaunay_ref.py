"""An oracle for the Delaunay triangulation that is independent of the library, and the inputs the star path is
tested on (tests/test_delaunay_star.py, tests/test_delaunay_star_gpu.py).

oracle(xy): the definition, in exact rational arithmetic (fractions.Fraction of the doubles, brought to one common
denominator so that the determinants are integer).  A triangle is Delaunay iff it is counter-clockwise and no point
is strictly inside its circumcircle: O(n^4), for n <= 30.  Returns the canonical list (each triangle starting at its
smallest vertex, orientation kept, sorted) or the string "ties" when some point is exactly on the circle of a
listed triangle (the triangulation is then not unique)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np


def _exact_ints(xy):
    fr = [[Fraction(float(v)) for v in p] for p in np.asarray(xy, np.float64)]
    den = 1
    for p in fr:
        for v in p:
            den = den * v.denominator // math.gcd(den, v.denominator)
    return [(int(p[0] * den), int(p[1] * den)) for p in fr]


def _orient(a, b, c):
    return (a[0] - c[0]) * (b[1] - c[1]) - (a[1] - c[1]) * (b[0] - c[0])


def _incircle(a, b, c, d):
    adx, ady, bdx, bdy, cdx, cdy = a[0] - d[0], a[1] - d[1], b[0] - d[0], b[1] - d[1], c[0] - d[0], c[1] - d[1]
    return ((adx * adx + ady * ady) * (bdx * cdy - cdx * bdy) + (bdx * bdx + bdy * bdy) * (cdx * ady - adx * cdy) +
            (cdx * cdx + cdy * cdy) * (adx * bdy - bdx * ady))


def canonical(tris):
    out = []
    for t in tris:
        k = int(np.argmin(t))
        out.append((t[k], t[(k + 1) % 3], t[(k + 2) % 3]))
    return np.asarray(sorted(out), np.int32).reshape(-1, 3)


def oracle(xy):
    pts = _exact_ints(xy)
    n = len(pts)
    assert n <= 30
    tris, ties = [], False
    for i in range(n):
        for j in range(i + 1, n):
            for k in range(j + 1, n):
                o = _orient(pts[i], pts[j], pts[k])
                if o == 0:
                    continue
                t = (i, j, k) if o > 0 else (i, k, j)
                empty, on = True, False
                for m in range(n):
                    if m in t:
                        continue
                    s = _incircle(pts[t[0]], pts[t[1]], pts[t[2]], pts[m])
                    if s > 0:
                        empty = False
                        break
                    on |= s == 0
                if empty:
                    tris.append(t)
                    ties |= on
    return "ties" if ties else canonical(tris)


def sweep(xy):
    """The library's host sweep (delaunay2d) through its test hook: (tris [T, 3], hull_size, skipped), or None for
    collinear input."""
    from deftri import capi
    lib = capi.load()
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    tris = np.zeros((2 * len(xy) + 1, 3), np.int32)
    hull, skipped = C.c_int32(), C.c_int32()
    nt = lib.deftri_debug_delaunay_sweep(len(xy), xy.ctypes.data_as(C.POINTER(C.c_double)), len(tris),
                                         tris.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(hull), C.byref(skipped))
    if nt == -6:
        return None
    assert nt >= 0, nt
    return tris[:nt].copy(), hull.value, skipped.value


def still_valid(xy, tris):
    """delaunay_still_valid, the structure memo's exact certificate."""
    from deftri import capi
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    tris = np.ascontiguousarray(tris, np.int32)
    return capi.load().deftri_debug_delaunay_still_valid(len(xy), xy.ctypes.data_as(C.POINTER(C.c_double)), len(tris),
                                                         tris.ctypes.data_as(C.POINTER(C.c_int32)))


# ---- inputs ------------------------------------------------------------------------------------------------------
def widen(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float64))


def gaussian(n, seed=0):
    """The workload's cloud (sim.generate_points: a dense centre, empty outskirts), float32 widened to double."""
    from deftri import sim
    return widen(sim.generate_points(n, seed=seed)[0][:, :2])


def uniform(n, seed=0):
    return widen(np.random.RandomState(seed).uniform(0.0, 1.0, (n, 2)))


def jittered_lattice(side=20, jitter=1e-3, seed=1):
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    return g + np.random.RandomState(seed).uniform(-jitter, jitter, g.shape)


def circle_with_centre(n=100, seed=2):
    """A star of n neighbours: above the device's 64."""
    rs = np.random.RandomState(seed)
    a = 2 * np.pi * (np.arange(n) + rs.uniform(0.0, 0.3, n)) / n
    r = 1.0 + rs.uniform(-1e-3, 1e-3, n)
    return np.concatenate([[[0.0, 0.0]], np.stack([r * np.cos(a), r * np.sin(a)], 1)])


def two_clusters(n=300, seed=3):
    """Two dense clusters far apart: nearly every cell between them is empty."""
    p = np.random.RandomState(seed).normal(0.0, 1.0, (n, 2))
    p[1::2] += (1e4, 5e3)
    return p


def strip(n=500, seed=4):
    return np.random.RandomState(seed).uniform(0.0, 1.0, (n, 2)) * (200.0, 1.0)


def crowded_cell(seed=5):
    """70 points packed into one cell's extent, and 3 far corners."""
    p = 0.5 + 1e-3 * np.random.RandomState(seed).uniform(0.0, 1.0, (70, 2))
    return np.concatenate([p, [[-50.0, -40.0], [60.0, -45.0], [3.0, 70.0]]])


def near_tie(seed=6):
    """Four nearly cocircular points (the fourth 2^-50 off the circle) inside a ring of 60: the in-circle filter
    cannot decide the square's diagonal; no predicate is exactly zero."""
    rs = np.random.RandomState(seed)
    r, a = rs.uniform(3.0, 6.0, 60), rs.uniform(0.0, 2 * np.pi, 60)
    ring = np.stack([0.5 + r * np.cos(a), 0.5 + r * np.sin(a)], 1)
    return np.concatenate([[[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0 + 2.0 ** -50]], ring])


def exact_lattice(side=8):
    return np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)


def with_duplicate(n=50, seed=7):
    p = gaussian(n, seed)
    p[31] = p[7]
    return p


def line(n=40):
    t = np.arange(n, dtype=np.float64)
    return np.stack([0.25 * t, 0.5 * t], 1)


# name -> points: the inputs without tie or duplicate (the stars are built, nothing falls back)
CLEAN = {
    "gaussian65": lambda: gaussian(65, 1),
    "gaussian300": lambda: gaussian(300, 2),
    "gaussian2000": lambda: gaussian(2000, 3),
    "uniform2000": lambda: uniform(2000, 4),
    "jittered_lattice": jittered_lattice,
    "circle_with_centre": circle_with_centre,
    "two_clusters": two_clusters,
    "strip": strip,
}
RANDOM_CLOUDS = ("gaussian65", "gaussian300", "gaussian2000", "uniform2000")
