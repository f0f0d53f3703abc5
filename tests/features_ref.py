"""FAST::extract (reference Modules/Features/FAST.cc:81-118, FAST.h:52-97) restated in numpy, stage by stage,
for the tests of deftri_fast_extract.  It shares no code with csrc/: the library is held to it exactly.

OpenCV's parts (the 8-bit bilinear resize, FAST-9/16 with non-maximum suppression, fastAtan2) follow their
definitions as include/deftri.h states them; OpenCV itself is not a test dependency.

Also the scene generator: seeded 8-bit images of rectangles, discs and gradients with low noise, a few
saturated blobs, and an optional border mask (a filled frame).
"""
import math

import numpy as np

F = np.float32
EDGE = 16                     # EDGE_THRESHOLD - 3
HALF_PATCH = 15
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
        (-3, 1), (-2, 2), (-1, 3)]         # (dx, dy), the Bresenham circle of radius 3 in ring order


def cv_round(v):
    """cvRound: to nearest, ties to even."""
    return int(np.rint(v))


# ---- 1. scale tables (FAST.h:54-78) ---------------------------------------------------------------
def scale_tables(n_scales, scale_factor, n_max_features):
    f = F(scale_factor)
    scale = [F(1.0)]
    for _ in range(1, n_scales):
        scale.append(F(scale[-1] * f))
    inv = [F(F(1.0) / s) for s in scale]
    factor = F(F(1.0) / f)
    desired = F(F(F(n_max_features) * F(F(1) - factor)) / F(F(1) - F(math.pow(float(factor), float(n_scales)))))
    per_level, total = [], 0
    for _ in range(n_scales - 1):
        per_level.append(cv_round(desired))
        total += per_level[-1]
        desired = F(desired * factor)
    per_level.append(max(n_max_features - total, 0))
    return scale, inv, per_level


def umax_table():
    """FAST.h:82-96."""
    umax = [0] * (HALF_PATCH + 1)
    vmax = int(math.floor(float(F(F(HALF_PATCH) * np.sqrt(F(2.0)) / F(2) + F(1)))))
    vmin = int(math.ceil(float(F(F(HALF_PATCH) * np.sqrt(F(2.0)) / F(2)))))
    for v in range(vmax + 1):
        umax[v] = cv_round(math.sqrt(HALF_PATCH * HALF_PATCH - v * v))
    v0 = 0
    for v in range(HALF_PATCH, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


# ---- 2. pyramid (FAST.cc:120-139) -------------------------------------------------------------------
def _axis_taps(src, dst):
    scale = src / dst                                        # double
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(F)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F)).astype(F)
    low = s < 0
    s[low] = 0; f[low] = 0
    high = s >= src - 1
    s[high] = src - 1; f[high] = 0
    s1 = np.where(high, s, s + 1)
    a0 = np.rint((F(1.0) - f).astype(F) * F(2048)).astype(np.int64)
    a1 = np.rint(f * F(2048)).astype(np.int64)
    return s, s1, a0, a1


def resize_linear_u8(src, dst_rows, dst_cols):
    """cv::resize(src, Size(dst_cols, dst_rows), INTER_LINEAR) on 8-bit data."""
    src = src.astype(np.int64)
    xs, xs1, a0, a1 = _axis_taps(src.shape[1], dst_cols)
    ys, ys1, b0, b1 = _axis_taps(src.shape[0], dst_rows)
    h = src[:, xs] * a0[None, :] + src[:, xs1] * a1[None, :]              # [src rows, dst cols]
    h0, h1 = h[ys, :], h[ys1, :]
    out = (((b0[:, None] * (h0 >> 4)) >> 16) + ((b1[:, None] * (h1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def pyramid(image, inv):
    rows, cols = image.shape
    levels = [image.copy()]
    for l in range(1, len(inv)):
        levels.append(resize_linear_u8(levels[-1], cv_round(F(rows) * inv[l]), cv_round(F(cols) * inv[l])))
    return levels


# ---- 3. cells (:141-203) ------------------------------------------------------------------------------
def fast_scores(cell):
    """s of every pixel of `cell` that has its whole ring inside: the maximum over the 16 arcs of 9 contiguous
    ring pixels of the arc's minimum of p_i - c, and of c - p_i.  [rows - 6, cols - 6]."""
    c = cell.astype(np.int32)
    rows, cols = c.shape
    centre = c[3:rows - 3, 3:cols - 3]
    d = np.stack([c[3 + dy:rows - 3 + dy, 3 + dx:cols - 3 + dx] - centre for dx, dy in RING])      # [16, ., .]
    best = np.full(centre.shape, -255, np.int32)
    for k in range(16):
        arc = d[[(k + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))
    return best


def fast_cell(cell, th):
    """cv::FAST(cell, keys, th, true): (x, y, response) in row-major order."""
    rows, cols = cell.shape
    if rows < 7 or cols < 7:
        return []
    s = fast_scores(cell)
    resp = np.zeros((rows, cols), np.int32)                    # 0: no corner at th, or the 3-pixel margin
    resp[3:rows - 3, 3:cols - 3] = np.where(s > th, s - 1, 0)
    keys = []
    for y, x in zip(*np.nonzero(resp)):
        r = resp[y, x]
        nb = resp[y - 1:y + 2, x - 1:x + 2].copy()
        nb[1, 1] = -1
        if r > nb.max():
            keys.append((int(x), int(y), int(r)))
    return keys


def level_candidates(img, th_fast, min_th_fast):
    """vToDistributeKeys of one level: [(x, y, response)] relative to the border, and (fallback cells, cells
    empty after the fallback)."""
    min_bx = min_by = EDGE
    max_bx, max_by = img.shape[1] - EDGE, img.shape[0] - EDGE
    width, height = F(max_bx - min_bx), F(max_by - min_by)
    W = F(30)
    n_cols, n_rows = int(width / W), int(height / W)
    w_cell, h_cell = int(math.ceil(float(F(width / F(n_cols))))), int(math.ceil(float(F(height / F(n_rows)))))
    out, fallback, empty = [], 0, 0
    for i in range(n_rows):
        ini_y = min_by + i * h_cell
        max_y = ini_y + h_cell + 6
        if ini_y >= max_by - 3:
            continue
        max_y = min(max_y, max_by)
        for j in range(n_cols):
            ini_x = min_bx + j * w_cell
            max_x = ini_x + w_cell + 6
            if ini_x >= max_bx - 6:
                continue
            max_x = min(max_x, max_bx)
            cell = img[ini_y:max_y, ini_x:max_x]
            keys = fast_cell(cell, th_fast)
            if not keys:
                fallback += 1
                keys = fast_cell(cell, min_th_fast)
                if not keys:
                    empty += 1
            out += [(x + j * w_cell, y + i * h_cell, r) for x, y, r in keys]
    return out, fallback, empty


# ---- 4. distributeOctTree (:243-434) ----------------------------------------------------------------
class _Node:
    __slots__ = ("x0", "y0", "x1", "y1", "keys", "no_more", "born")

    def __init__(self, x0, y0, x1, y1):
        self.x0, self.y0, self.x1, self.y1 = x0, y0, x1, y1      # UL, UR.x, BL.y
        self.keys, self.no_more, self.born = [], False, -1


def _divide(n):
    half_x = int(math.ceil(float(F(F(n.x1 - n.x0) / F(2)))))
    half_y = int(math.ceil(float(F(F(n.y1 - n.y0) / F(2)))))
    xm, ym = n.x0 + half_x, n.y0 + half_y
    ch = [_Node(n.x0, n.y0, xm, ym), _Node(xm, n.y0, n.x1, ym), _Node(n.x0, ym, xm, n.y1), _Node(xm, ym, n.x1, n.y1)]
    for k in n.keys:
        if k[0] < xm:
            ch[0 if k[1] < ym else 2].keys.append(k)
        else:
            ch[1 if k[1] < ym else 3].keys.append(k)
    for c in ch:
        c.no_more = len(c.keys) == 1
    return ch


def distribute_oct_tree(cands, width, height, N, stats=None):
    """cands [(x, y, response)] -> the kept ones in the order of the reference's list.  Equal node sizes in
    the sorted branch: the most recently created node first (the project's stated choice).  stats, if given,
    receives how the loop ended: 'sorted' (inside the sorted branch at N), 'ties' (equal sizes met there),
    'single' (every node holds one point)."""
    # round(): half away from zero; the quotient is positive
    n_ini = int(math.floor(float(F(F(width) / F(height))) + 0.5))
    assert n_ini >= 1
    hx = F(F(width) / F(n_ini))
    nodes = []
    for i in range(n_ini):
        nodes.append(_Node(int(F(hx * F(i))), 0, int(F(hx * F(i + 1))), height))
    for k in cands:
        nodes[int(F(F(k[0]) / hx))].keys.append(k)
    born = [0]

    def push_front(lst, n):
        n.born = born[0]
        born[0] += 1
        lst.insert(0, n)

    lst = []
    for n in nodes:                       # creation order = list order here
        n.born = born[0]
        born[0] += 1
        if len(n.keys) == 1:
            n.no_more = True
        if n.keys:
            lst.append(n)
    stats = stats if stats is not None else {}
    finish = False
    while not finish:
        prev_size = len(lst)
        to_expand = []
        n_to_expand = 0
        for n in list(lst):               # nodes pushed to the front during the pass are not visited
            if n.no_more:
                continue
            for c in _divide(n):
                if c.keys:
                    push_front(lst, c)
                    if len(c.keys) > 1:
                        n_to_expand += 1
                        to_expand.append(c)
            lst.remove(n)
        if len(lst) >= N or len(lst) == prev_size:
            finish = True
            if len(lst) == prev_size and all(len(n.keys) == 1 for n in lst):
                stats["single"] = True
        elif len(lst) + n_to_expand * 3 > N:
            while not finish:
                prev_size = len(lst)
                prev, to_expand = to_expand, []
                prev.sort(key=lambda n: (len(n.keys), n.born))
                sizes = [len(n.keys) for n in prev]
                for j in range(len(prev) - 1, -1, -1):
                    if j > 0 and sizes[j] == sizes[j - 1]:
                        stats["ties"] = True
                    for c in _divide(prev[j]):
                        if c.keys:
                            push_front(lst, c)
                            if len(c.keys) > 1:
                                to_expand.append(c)
                    lst.remove(prev[j])
                    if len(lst) >= N:
                        stats["sorted"] = True
                        break
                if len(lst) >= N or len(lst) == prev_size:
                    finish = True
    kept = []
    for n in lst:
        best = n.keys[0]
        for k in n.keys[1:]:
            if k[2] > best[2]:
                best = k
        kept.append(best)
    return kept


# ---- 5. mask (:223-234, :470-528) -------------------------------------------------------------------
def base_mask(image, border_mask=None):
    m = image > 240
    if border_mask is not None:
        assert border_mask.shape == image.shape
        m = m | (border_mask != 0)
    return m


def mask_side(level):
    factor = F(2.5 / 1.5)
    return int(math.ceil(float(F(F(2 ** (level + 1)) * factor)))) * 2 + 5


def mask_read(base, level, x, y):
    """The dilated mask of `level` at (x, y): any base pixel in the side x side window clipped to the image."""
    h = (mask_side(level) - 1) // 2
    return bool(base[max(y - h, 0):y + h + 1, max(x - h, 0):x + h + 1].any())


# ---- 6. orientation (:443-467) ----------------------------------------------------------------------
def fast_atan2(y, x):
    y, x = F(y), F(x)
    ax, ay = np.abs(x), np.abs(y)
    eps = F(2.220446049250313e-16)
    p1, p3, p5, p7 = F(57.283627), F(-18.667446), F(8.9140005), F(-2.5397246)

    def poly(c):
        c2 = c * c                                            # float32 throughout: one rounding per operation
        return (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c

    if ax >= ay:
        a = poly(F(ay / F(ax + eps)))
    else:
        a = F(F(90.0) - poly(F(ax / F(ay + eps))))
    if x < 0:
        a = F(F(180.0) - a)
    if y < 0:
        a = F(F(360.0) - a)
    return a


def ic_angle(img, x, y, umax):
    p = img.astype(np.int64)
    m01 = m10 = 0
    for v in range(-HALF_PATCH, HALF_PATCH + 1):
        d = umax[abs(v)]
        row = p[y + v, x - d:x + d + 1]
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += v * int(row.sum())
    return fast_atan2(m01, m10)


# ---- 7. the whole of extract (:81-118) --------------------------------------------------------------
def extract(image, n_scales, scale_factor, n_max_features, th_fast, min_th_fast, max_keys, border_mask=None):
    """Returns a dict: uv, octave, angle, response, size (arrays), report (the per-level counts of
    deftri_fast_report), and levels / candidates / stats for the stage tests."""
    scale, inv, per_level = scale_tables(n_scales, scale_factor, n_max_features)
    levels = pyramid(image, inv)
    base = base_mask(image, border_mask)
    umax = umax_table()
    rep = {k: [] for k in ("level_cols", "level_rows", "features_per_level", "n_candidates", "n_octree", "n_after_mask",
                           "n_fallback_cells", "n_empty_cells", "n_truncated")}
    uv, octave, angle, response, size = [], [], [], [], []
    candidates, stats, masked_by = [], [], []
    for l, img in enumerate(levels):
        cands, fallback, empty = level_candidates(img, th_fast, min_th_fast)
        candidates.append(cands)
        st = {}
        kept = distribute_oct_tree(cands, img.shape[1] - 2 * EDGE, img.shape[0] - 2 * EDGE, per_level[l], st)
        stats.append(st)
        after, truncated = 0, 0
        for kx, ky, r in kept:
            x, y = kx + EDGE, ky + EDGE
            if mask_read(base, l, x, y):
                masked_by.append((l, x, y))
                continue
            after += 1
            if len(octave) >= max_keys:
                truncated += 1
                continue
            uv.append((F(F(x) * scale[l]), F(F(y) * scale[l])))
            octave.append(l)
            angle.append(ic_angle(img, x, y, umax))
            response.append(F(r))
            size.append(F(int(F(F(31) * scale[l]))))
        for k, v in (("level_cols", img.shape[1]), ("level_rows", img.shape[0]), ("features_per_level", per_level[l]),
                     ("n_candidates", len(cands)), ("n_octree", len(kept)), ("n_after_mask", after), ("n_fallback_cells", fallback),
                     ("n_empty_cells", empty), ("n_truncated", truncated)):
            rep[k].append(int(v))
    rep["n_levels"] = n_scales
    rep["n_keys"] = len(octave)
    return {"uv": np.array(uv, F).reshape(-1, 2), "octave": np.array(octave, np.int32), "angle": np.array(angle, F),
            "response": np.array(response, F), "size": np.array(size, F), "report": rep, "levels": levels,
            "candidates": candidates, "stats": stats, "masked": masked_by}


# ---- scenes -------------------------------------------------------------------------------------------
def make_scene(rows, cols, seed, n_shapes=None, n_blobs=3, frame=0):
    """A seeded 8-bit image [rows, cols] of rectangles, discs and gradients with low noise and n_blobs saturated
    blobs, and a border mask (a filled frame `frame` pixels wide; None for frame == 0)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    img = 60.0 + 50.0 * xx / cols + 30.0 * yy / rows
    n_shapes = n_shapes if n_shapes is not None else max(rows * cols // 500, 12)
    # the lower right quarter stays smooth: cells that fall back and cells that stay empty
    for _ in range(n_shapes):
        cx, cy = rng.integers(0, cols), rng.integers(0, rows)
        if cx > cols * 0.6 and cy > rows * 0.6:
            continue
        level = float(rng.integers(20, 200))
        if rng.random() < 0.5:
            w, h = rng.integers(4, 28, 2)
            img[max(cy - h, 0):cy + h, max(cx - w, 0):cx + w] = level
        else:
            r = rng.integers(3, 16)
            img[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = level
    # a faint texture in part of the smooth quarter: corners only min_th_fast finds
    for _ in range(6):
        cx, cy = rng.integers(int(cols * 0.62), cols - 4), rng.integers(int(rows * 0.62), rows - 4)
        w, h = rng.integers(3, 9, 2)
        img[cy - h:cy + h, cx - w:cx + w] += 7.0
    img = img + rng.normal(0.0, 0.6, img.shape)
    img = np.clip(img, 0, 235)
    for _ in range(n_blobs):
        cx, cy = rng.integers(10, int(cols * 0.6)), rng.integers(10, int(rows * 0.6))
        r = rng.integers(2, 6)
        img[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 250.0
    image = np.rint(img).astype(np.uint8)
    border = None
    if frame:
        border = np.zeros((rows, cols), np.uint8)
        border[:frame, :] = 255; border[-frame:, :] = 255; border[:, :frame] = 255; border[:, -frame:] = 255
    return image, border
