"""TEST INFRASTRUCTURE ONLY: synthetic scenes for searchForInitializaion (numpy alone, seeded).

A scene is a dict: grid (deftri_feature_grid's fields), uv1 / octave1 / desc1 (reference frame), uv2 /
octave2 / desc2 (current frame), th, radius, and for the hand-placed ones `expect`, the matches the
reference's loop gives.  Current keypoints are the reference keypoints plus a shift smaller than the radius;
descriptors are random 256-bit strings, matched ones with a few bits flipped.
"""
import numpy as np

REALCOLON = dict(cols=64, rows=48, min_col=0.0, min_row=0.0, max_col=1440.0, max_row=1080.0, n_scales=8, scale_factor=1.2)
SMALL = dict(cols=16, rows=12, min_col=0.0, min_row=0.0, max_col=320.0, max_row=240.0, n_scales=8, scale_factor=1.2)


def flip_bits(desc, bits):
    """A copy of a 32-byte descriptor with the given bit positions flipped."""
    d = np.array(desc, np.uint8).copy()
    for b in bits:
        d[int(b) // 8] ^= np.uint8(1 << (int(b) % 8))
    return d


def first_bits(k):
    """A descriptor with its first k bits set: distance k to the zero descriptor."""
    return flip_bits(np.zeros(32, np.uint8), range(k))


def _pack(grid, uv1, o1, d1, uv2, o2, d2, th, radius, expect=None):
    s = dict(grid=grid, uv1=np.asarray(uv1, np.float32).reshape(-1, 2), octave1=np.asarray(o1, np.int32),
             desc1=np.asarray(d1, np.uint8).reshape(-1, 32), uv2=np.asarray(uv2, np.float32).reshape(-1, 2),
             octave2=np.asarray(o2, np.int32), desc2=np.asarray(d2, np.uint8).reshape(-1, 32), th=int(th), radius=float(radius))
    if expect is not None:
        s["expect"] = np.asarray(expect, np.int32)
    return s


def args(s):
    return (s["grid"], s["uv1"], s["octave1"], s["desc1"], s["uv2"], s["octave2"], s["desc2"], s["th"], s["radius"])


def random_scene(n, grid, radius, th=100, seed=0):
    """n keypoints over the whole image (the borders included); the current frame is a permutation of the
    shifted reference keypoints; a fifth of either frame is of a coarser octave; a tenth of the current
    descriptors are unrelated, a tenth have a near-duplicate rival."""
    rng = np.random.default_rng(seed)
    uv1 = rng.uniform(0, 1, (n, 2)) * [grid["max_col"], grid["max_row"]]
    shift = rng.uniform(-0.9 * radius, 0.9 * radius, (n, 2))
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d2 = d1.copy()
    for i in range(n):
        kind = rng.integers(0, 10)
        if kind == 0:
            d2[i] = rng.integers(0, 256, 32, dtype=np.uint8)
        else:
            d2[i] = flip_bits(d1[i], rng.choice(256, rng.integers(0, 12), replace=False))
    uv2 = uv1 + shift
    # rivals: a second current keypoint next to some, with a descriptor almost as close
    nr = max(n // 10, 1)
    who = rng.choice(n, nr, replace=False)
    uv2 = np.concatenate([uv2, uv2[who] + rng.uniform(-1, 1, (nr, 2))])
    d2 = np.concatenate([d2, np.stack([flip_bits(d2[w], rng.choice(256, rng.integers(0, 3), replace=False)) for w in who])])
    perm = rng.permutation(len(uv2))
    uv2, d2 = uv2[perm], d2[perm]
    o1 = np.where(rng.uniform(size=n) < 0.2, rng.integers(1, 4, n), 0)
    o2 = np.where(rng.uniform(size=len(uv2)) < 0.2, rng.integers(1, 4, len(uv2)), 0)
    return _pack(grid, uv1, o1, d1, uv2, o2, d2, th, radius)


def window_scene(n_inside, n_total=None, seed=0, spread_y=30.0):
    """One reference keypoint at (697.5, 500) on the Realcolon grid, radius 25, and n_total current keypoints
    whose x lies in one grid column (686.25 <= x < 708.75) around it; exactly n_inside of them (when n_total is
    given) lie inside the window, the others above or below it.  n_total None: n_inside keypoints spread over
    +-spread_y, of which those within +-25 pass.  A few further reference keypoints far away."""
    rng = np.random.default_rng(seed)
    x0, y0, radius = 697.5, 500.0, 25.0
    if n_total is None:
        n2 = n_inside
        uv2 = np.stack([rng.uniform(687.0, 708.0, n2), y0 + rng.uniform(-spread_y, spread_y, n2)], 1)
    else:
        n2 = n_total
        dy = np.concatenate([rng.uniform(-24.0, 24.0, n_inside),
                             rng.choice([-1.0, 1.0], n2 - n_inside) * rng.uniform(26.0, 33.0, n2 - n_inside)])
        uv2 = np.stack([rng.uniform(687.0, 708.0, n2), y0 + dy], 1)
    d1 = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    d2[n2 // 2] = flip_bits(d1[0], [3, 77, 200])                   # the match, inside the window
    uv2[n2 // 2, 1] = y0 + 3.0
    d2[n2 // 3] = flip_bits(d1[0], range(40, 100))                 # a distant second
    uv1 = np.array([[x0, y0], [100.0, 100.0], [1300.0, 900.0], [697.5, 700.0]])
    perm = rng.permutation(n2)
    return _pack(REALCOLON, uv1, np.zeros(4), d1, uv2[perm], np.zeros(n2), d2[perm], 100, radius)


def acceptance_scene():
    """257 x 257 reference keypoints, each alone with two candidates at distances (b, s) in [0, 256]^2:
    reference keypoint b * 257 + s has the zero descriptor, its candidates b and s leading bits set."""
    grid = dict(cols=64, rows=64, min_col=0.0, min_row=0.0, max_col=4096.0, max_row=4096.0, n_scales=8, scale_factor=1.2)
    b, s = np.divmod(np.arange(257 * 257), 257)
    uv1 = np.stack([20.0 + 8.0 * s, 20.0 + 8.0 * b], 1)
    uv2 = np.concatenate([uv1 + [0.5, 0.0], uv1 + [0.0, 0.5]])
    table = np.stack([first_bits(k) for k in range(257)])
    d2 = np.concatenate([table[b], table[s]])
    n = len(uv1)
    sc = _pack(grid, uv1, np.zeros(n), np.zeros((n, 32), np.uint8), uv2, np.zeros(2 * n), d2, 256, 2.0)
    sc["b"], sc["s"] = b, s
    return sc


def quirk_scenes():
    """name -> scene with `expect`, each placed by hand on the Realcolon grid (radius 25, th 100 unless noted)."""
    rng = np.random.default_rng(11)
    rd = lambda k=1: rng.integers(0, 256, (k, 32), dtype=np.uint8)
    G = REALCOLON
    out = {}
    # x = 1429 rounds to column 64: in no cell, never matched although it is the only candidate; x = 1428 is
    a = rd(2)
    out["last_half_cell_x"] = _pack(G, [[1420, 500], [1420, 800]], [0, 0], a,
                                    [[1429, 500], [1428, 800]], [0, 0], [flip_bits(a[0], [1]), flip_bits(a[1], [1])], 100, 25,
                                    [-1, 1])
    # the same at the bottom: 1080 rows, 48 cells, y >= 1068.75
    a = rd(2)
    out["last_half_cell_y"] = _pack(G, [[500, 1060], [800, 1060]], [0, 0], a,
                                    [[500, 1069], [800, 1068]], [0, 0], [flip_bits(a[0], [1]), flip_bits(a[1], [1])], 100, 25,
                                    [-1, 1])
    a = rd(2)
    out["reference_octave_1"] = _pack(G, [[300, 300], [600, 300]], [1, 0], a, [[302, 301], [602, 301]], [0, 0],
                                      [flip_bits(a[0], [5]), flip_bits(a[1], [5])], 100, 25, [-1, 1])
    # a current keypoint of octave 2 is no candidate for an octave-0 reference; octave 1 is
    a = rd(2)
    out["current_octave_2"] = _pack(G, [[300, 300], [600, 300]], [0, 0], a, [[302, 301], [602, 301]], [2, 1],
                                    [flip_bits(a[0], [5]), flip_bits(a[1], [5])], 100, 25, [-1, 1])
    a = rd(1)
    out["tie_for_best"] = _pack(G, [[300, 300]], [0], a, [[302, 301], [297, 299], [305, 305]], [0, 0, 0],
                                [flip_bits(a[0], [5, 9]), flip_bits(a[0], [100, 200]), flip_bits(a[0], range(60))], 100, 25, [-1])
    a = rd(2)
    d20, d21 = flip_bits(a[0], range(20)), flip_bits(a[1], range(21))
    out["best_equals_th"] = _pack(G, [[300, 300], [600, 300]], [0, 0], a, [[302, 301], [602, 301]], [0, 0], [d20, d21], 20, 25,
                                  [0, -1])
    # the window leaves the image on each of the four sides (and at a corner)
    a = rd(5)
    uv1 = np.array([[5, 500], [1425, 500], [700, 5], [700, 1060], [4, 4]], float)
    uv2 = uv1 + [[3, 2], [2, -3], [-2, 3], [3, 4], [2, 2]]
    out["window_leaves_image"] = _pack(G, uv1, np.zeros(5), a, uv2, np.zeros(5), [flip_bits(a[i], [i, 50]) for i in range(5)],
                                       100, 25, [0, 1, 2, 3, 4])
    # nothing makes the matches one-to-one
    a = rd(1)
    out["two_to_one"] = _pack(G, [[300, 300], [310, 305]], [0, 0], [flip_bits(a[0], [1]), flip_bits(a[0], [2, 3])],
                              [[305, 302]], [0], a, 100, 25, [0, 0])
    # complementary descriptors: distance 256 never becomes the best, whatever th; neither does 255
    a = rd(2)
    out["distance_256"] = _pack(G, [[300, 300], [600, 300]], [0, 0], a, [[302, 301], [602, 301]], [0, 0],
                                [~a[0], flip_bits(~a[1], [7])], 256, 25, [-1, -1])
    return out
