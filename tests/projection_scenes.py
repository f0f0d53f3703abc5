"""TEST INFRASTRUCTURE ONLY: synthetic scenes for guidedMatching, searchWithProjection and
Map::updateOrientationAndDescriptor (numpy alone, seeded).

A projection scene is a dict with the arguments of Context.search_with_projection: grid, Tcw, kb8, uv2 /
octave2 / desc2 / slot_point (the frame), pos / normal / min_dist / max_dist / desc (the map points), th.
Map points are placed in the frame's camera coordinates and moved to the world with the fp64 pose; normals
and invariance distances are chosen so that a point lands in the branch that is wanted of it; keypoints are
placed around the fp64 projections.
"""
import numpy as np

from deftri import matching
from deftri.mapmodel import SE3f, mat_from_quat
import matching_scenes as ms

GRID = ms.REALCOLON
KB8 = np.array([717.2, 717.5, 735.4, 552.8, -0.13, -0.01, 0.003, -0.001], np.float32)
N_SCALES, FACTOR = GRID["n_scales"], GRID["scale_factor"]


def pose():
    q = np.array([0.02, -0.03, 0.01, 1.0]); q /= np.linalg.norm(q)
    return SE3f(mat_from_quat(q).astype(np.float32), np.array([0.01, -0.02, 0.03], np.float32))


def to_world(T, pc):
    """World points of camera points under the float pose, in fp64."""
    return (np.asarray(pc, np.float64) - T.t.astype(np.float64)) @ T.R.astype(np.float64)


def centre(T):
    return -(T.R.astype(np.float64).T @ T.t.astype(np.float64))


def camera_points(rng, n, lo=0.08, hi=0.25, spread=0.55):
    z = rng.uniform(lo, hi, n)
    return np.stack([rng.uniform(-spread, spread, n) * z, rng.uniform(-spread * 0.7, spread * 0.7, n) * z, z], 1)


def normal_with_cos(rng, ray, cos):
    """A unit vector whose cosine with `ray` is `cos`."""
    r = ray / np.linalg.norm(ray)
    a = np.cross(r, rng.normal(size=3)); a /= np.linalg.norm(a)
    return cos * r + np.sqrt(max(1.0 - cos * cos, 0.0)) * a


def scale(octave):
    return float(matching.scale_factors(GRID)[octave])


def pack(T, uv2, o2, d2, slot, pos, normal, mn, mx, desc, th=60, grid=GRID, kb8=KB8):
    return dict(grid=grid, Tcw=T, kb8=kb8, uv2=np.asarray(uv2, np.float32).reshape(-1, 2), octave2=np.asarray(o2, np.int32),
                desc2=np.asarray(d2, np.uint8).reshape(-1, 32), slot_point=np.asarray(slot, np.int32),
                pos=np.asarray(pos, np.float32).reshape(-1, 3), normal=np.asarray(normal, np.float32).reshape(-1, 3),
                min_dist=np.asarray(mn, np.float32), max_dist=np.asarray(mx, np.float32),
                desc=np.asarray(desc, np.uint8).reshape(-1, 32), th=int(th))


def args(s):
    return (s["grid"], s["Tcw"], s["kb8"], s["uv2"], s["octave2"], s["desc2"], s["slot_point"], s["pos"], s["normal"],
            s["min_dist"], s["max_dist"], s["desc"], s["th"])


def ref(s, dtype=np.float32):
    return matching.search_with_projection_ref(*args(s), dtype=dtype)


def point_for(rng, T, pc, cos, octave_ratio):
    """(world position, normal, min_dist, max_dist) of a camera point seen under view cosine `cos` whose
    log(max / dist) / log(1.2) is `octave_ratio`; min_dist = max_dist / 1.2^7."""
    X = to_world(T, pc)
    ray = X - centre(T)
    mx = np.linalg.norm(ray) * FACTOR ** octave_ratio
    return X, normal_with_cos(rng, ray, cos), mx / FACTOR ** (N_SCALES - 1), mx


def margin_scene(n, seed):
    """n map points over the image, in every branch of searchWithProjection: a tenth seen from the side (view
    cosine 0.3), a tenth outside the invariance distances, a tenth with an octave ratio above nScales - 1 (the clamp to
    nScales), a third seen head-on (cosine 0.9995, the narrow radius), the rest at cosine 0.8; octave ratios are
    k + 0.5.  Every searched point gets one keypoint with its descriptor (a few bits flipped) at 0.2 - 0.6 of its
    radius, a third of them a rival at the same place with a near-equal descriptor, a third a keypoint outside
    the window at 1.4 of the radius; a tenth of the frame's slots are occupied.  The scene is redrawn whole until
    the fp64 restatement decides nothing within the margins of margins_ok; every redraw has n points."""
    for attempt in range(200):
        rng = np.random.default_rng(1000 * seed + attempt)
        T = pose()
        pc = camera_points(rng, n)
        kind = rng.integers(0, 10, n)
        pos, nrm, mn, mx = [], [], [], []
        for i in range(n):
            cos = 0.3 if kind[i] == 0 else 0.9995 if kind[i] in (3, 4, 5) else 0.8
            # dist <= max needs a ratio >= 0, so the octaves are 1 .. 7; the clamp needs a min below max / 1.2^7
            ratio = rng.integers(0, N_SCALES - 1) + 0.5 if kind[i] != 2 else N_SCALES - 1 + 0.5 + rng.integers(0, 2)
            X, nr, lo, hi = point_for(rng, T, pc[i], cos, ratio)
            if kind[i] == 2:
                lo = hi / FACTOR ** 10
            if kind[i] == 1:                                    # too far: dist = 1.3 max
                lo, hi = lo / (1.3 * FACTOR ** ratio), hi / (1.3 * FACTOR ** ratio)
            pos.append(X); nrm.append(nr); mn.append(lo); mx.append(hi)
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        s = pack(T, np.zeros((0, 2)), [], np.zeros((0, 32)), [], pos, nrm, mn, mx, desc)
        r = ref(s, np.float64)                                  # no keypoints yet: uv, octave and radius
        uv2, o2, d2 = [], [], []
        for i in range(n):
            if r["status"][i] != matching.NO_CANDIDATES or i % 7 == 6:          # every seventh searched point: no candidate
                continue
            rad, oct_ = float(r["radius"][i]), int(r["predicted_octave"][i])
            place = lambda f: r["uv"][i] + f * rad * rng.choice([-1.0, 1.0], 2) * rng.uniform(0.5, 1.0, 2)
            uv2.append(place(rng.uniform(0.2, 0.6))); o2.append(np.clip(oct_ + rng.integers(-1, 2), 0, N_SCALES - 1))
            d2.append(ms.flip_bits(desc[i], rng.choice(256, rng.integers(0, 10), replace=False)))
            if i % 3 == 0:
                uv2.append(place(rng.uniform(0.2, 0.6))); o2.append(oct_)
                d2.append(ms.flip_bits(d2[-1], rng.choice(256, rng.integers(0, 4), replace=False)))
            if i % 3 == 1:
                f = rng.uniform(1.4, 1.6)
                uv2.append(r["uv"][i] + f * rad * np.array([1.0, 0.3]) * rng.choice([-1.0, 1.0])); o2.append(oct_)
                d2.append(desc[i])
        if not uv2:                                             # a lone point may be in a branch without a search
            uv2, o2, d2 = [[700.0, 500.0]], [0], [desc[0]]
        perm = rng.permutation(len(uv2))
        slot = np.where(rng.uniform(size=len(uv2)) < 0.1, -2, -1)
        s = pack(T, np.array(uv2)[perm], np.array(o2)[perm], np.array(d2)[perm], slot, pos, nrm, mn, mx, desc)
        if margins_ok(s, ref(s, np.float64)):
            s["attempt"] = attempt
            return s
    raise AssertionError("no scene within the margins")


def margins_ok(s, r64, px=0.01, rel=1e-3):
    """The fp64 restatement r64 of scene s decides nothing within `px` pixels of a window edge or of a
    cell-rounding boundary of the window's four corners, nor within `rel` of 0.5 / 0.998 (view cosine), of
    min / max (distance) or of an integer (octave ratio)."""
    g = s["grid"]
    vc, dist = r64["view_cos"], r64["dist"]
    ok = (np.abs(vc - 0.5) > rel) & (np.abs(vc - 0.998) > rel)
    seen = vc >= 0.5
    ok &= ~seen | ((np.abs(dist - s["min_dist"]) > rel * s["min_dist"]) & (np.abs(dist - s["max_dist"]) > rel * s["max_dist"]))
    ratio = r64["ratio"]
    has_ratio = np.isfinite(ratio)
    ok &= ~has_ratio | (np.abs(ratio - np.round(ratio)) > rel * np.maximum(np.abs(ratio), 1.0))
    searched = r64["radius"] > 0
    uv, rad = r64["uv"], r64["radius"]
    w = g["cols"] / (g["max_col"] - g["min_col"]); h = g["rows"] / (g["max_row"] - g["min_row"])
    for v, inv, lo in ((uv[:, 0] - rad, w, g["min_col"]), (uv[:, 0] + rad, w, g["min_col"]),
                       (uv[:, 1] - rad, h, g["min_row"]), (uv[:, 1] + rad, h, g["min_row"])):
        c = (v - lo) * inv
        ok &= ~searched | (np.abs(c - np.floor(c) - 0.5) > px * inv)
    d = np.abs(s["uv2"][None].astype(np.float64) - uv[:, None])                      # [n, n2, 2]
    near = np.abs(d - rad[:, None, None]) <= px                                      # on an edge line of the window ...
    reach = d < rad[:, None, None] + px                                              # ... within the other side's reach
    on_edge = ((near[:, :, 0] & reach[:, :, 1]) | (near[:, :, 1] & reach[:, :, 0])).any(axis=1)
    ok &= ~searched | ~on_edge
    return bool(ok.all())


def crowded_scene(n_keys=100, seed=0):
    """Three map points of predicted octave 7 (radius 4 * 1.2^7 = 14.3 px) around one pixel and n_keys keypoints of
    octaves 6 - 7 inside their windows: more than 64 candidates per wave."""
    rng = np.random.default_rng(seed)
    T = pose()
    pc = np.array([[0.0, 0.0, 0.15], [0.0002, 0.0, 0.15], [0.0, 0.0003, 0.15]])
    pts = [point_for(rng, T, p, 0.8, 6.5) for p in pc]
    desc = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    s = pack(T, np.zeros((0, 2)), [], np.zeros((0, 32)), [], *zip(*pts), desc)
    uv = ref(s, np.float64)["uv"]
    uv2 = uv[0] + rng.uniform(-9.0, 9.0, (n_keys, 2))
    d2 = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
    for i in range(3):
        d2[70 + 10 * i] = ms.flip_bits(desc[i], [i, 40 + i])
    return pack(T, uv2, rng.integers(6, 8, n_keys), d2, np.full(n_keys, -1), *zip(*pts), desc)


def point_scene(cos, ratio, keys, n_points=1, descs=None, slot=None, th=100):
    """n_points map points at one place, seen under view cosine `cos` with octave ratio `ratio`, and keypoints
    `keys`: (dx, dy, octave, bits) with the offset from the fp64 projection in units of getScaleFactor(predicted
    octave) and the first `bits` bits set.  descs: per point the number of leading bits set (default 0)."""
    rng = np.random.default_rng(3)
    T = pose()
    pt = point_for(rng, T, np.array([-0.01, 0.015, 0.18]), cos, ratio)
    desc = np.stack([ms.first_bits(b) for b in (descs or [0] * n_points)])
    cols = [[v] * n_points for v in pt]
    s = pack(T, np.zeros((0, 2)), [], np.zeros((0, 32)), [], *cols, desc)
    r = ref(s, np.float64)
    unit = scale(min(int(r["predicted_octave"][0]), N_SCALES - 1))
    uv2 = [r["uv"][0] + unit * np.array([dx, dy]) for dx, dy, _, _ in keys]
    s = pack(T, uv2, [k[2] for k in keys], [ms.first_bits(k[3]) for k in keys], slot if slot is not None else [-1] * len(keys),
             *cols, desc, th=th)
    s["uv64"] = r["uv"][0]
    return s


CHAIN_D = (3, 5, 7, 9, 11, 13, 16, 19, 22, 26, 30, 35, 40)


def chain_scene(n=10, order=None, occupied=(2, 5)):
    """n map points at one place (one window) and the keypoints CHAIN_D: keypoint j has its first CHAIN_D[j] bits set,
    map point i its first i % 2, so every point prefers the keypoints in the same order and each point's best is the
    first one the points before it left free; consecutive distances pass the 0.9 ratio test for either kind of
    point.  The keypoints `occupied` hold a map point beforehand.  order: a permutation of the points."""
    rng = np.random.default_rng(5)
    T = pose()
    X, nr, lo, hi = point_for(rng, T, np.array([0.01, -0.02, 0.2]), 0.8, 2.5)
    desc = np.stack([ms.first_bits(i % 2) for i in range(n)])
    if order is not None:
        desc = desc[np.asarray(order)]
    s = pack(T, np.zeros((0, 2)), [], np.zeros((0, 32)), [], [X] * n, [nr] * n, [lo] * n, [hi] * n, desc)
    r = ref(s, np.float64)
    m = len(CHAIN_D)
    uv2 = r["uv"][0] + rng.uniform(-0.5, 0.5, (m, 2)) * r["radius"][0]
    slot = np.full(m, -1); slot[list(occupied)] = -2
    s = pack(T, uv2, np.full(m, 2), np.stack([ms.first_bits(d) for d in CHAIN_D]), slot, [X] * n, [nr] * n, [lo] * n, [hi] * n,
             desc, th=100)
    free = [j for j in range(m) if j not in occupied]
    s["expect"] = np.array(free[:n], np.int32)                 # point i takes the i-th free keypoint
    return s


def descriptor_scene(n=300, n_kf=9, n_slots=320, seed=0):
    """n map points with 2 .. 9 observations (point p has 2 + p % 8) in n_kf keyframes around the scene, given in
    a shuffled keyframe order per point; observation descriptors are the point's own with 0 .. 60 bits flipped,
    redrawn per point until exactly one observation has the lowest median (from 4 observations on: with 2 or 3 the
    two closest observations always share theirs)."""
    rng = np.random.default_rng(seed)
    kf_T = []
    for k in range(n_kf):
        q = np.append(rng.normal(0, 0.05, 3), 1.0); q /= np.linalg.norm(q)
        R = mat_from_quat(q).astype(np.float32)
        c = np.array([0.05 * np.cos(k), 0.05 * np.sin(k), -0.02 * k], np.float32)
        kf_T.append(np.concatenate([R, (-(R @ c))[:, None]], 1))
    kf_T = np.array(kf_T, np.float32)
    pos = camera_points(rng, n, 0.15, 0.4).astype(np.float32)
    kf_slot_start = np.arange(n_kf + 1, dtype=np.int32) * n_slots
    kf_desc = rng.integers(0, 256, (n_kf * n_slots, 32), dtype=np.uint8)
    kf_octave = rng.integers(0, N_SCALES, n_kf * n_slots).astype(np.int32)
    slot_of = [rng.permutation(n_slots) for _ in range(n_kf)]                       # point p sits in slot slot_of[k][p]
    obs_start, obs_kf, obs_slot = [0], [], []
    for p in range(n):
        n_obs = 2 + p % 8
        kfs = rng.permutation(n_kf)[:n_obs]
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        while True:
            ds = np.stack([ms.flip_bits(base, rng.choice(256, rng.integers(0, 61), replace=False)) for _ in range(n_obs)])
            med = [int(np.sort(matching.hamming(np.repeat(ds[i][None], n_obs, 0), ds))[n_obs // 2]) for i in range(n_obs)]
            # with 2 or 3 observations the closest pair shares its median: the first of the two wins, on every path
            if med.count(min(med)) == 1 or n_obs < 4:
                break
        for k, d in zip(kfs, ds):
            kf_desc[k * n_slots + slot_of[k][p]] = d
            obs_kf.append(int(k)); obs_slot.append(int(slot_of[k][p]))
        obs_start.append(len(obs_kf))
    return dict(pos=pos, obs_start=np.array(obs_start, np.int32), obs_kf=np.array(obs_kf, np.int32),
                obs_slot=np.array(obs_slot, np.int32), kf_Tcw=kf_T, kf_slot_start=kf_slot_start, kf_desc=kf_desc,
                kf_octave=kf_octave, n_scales=N_SCALES, scale_factor=FACTOR)


def descriptor_args(s):
    return (s["pos"], s["obs_start"], s["obs_kf"], s["obs_slot"], s["kf_Tcw"], s["kf_slot_start"], s["kf_desc"], s["kf_octave"],
            s["n_scales"], s["scale_factor"])


def timing_scene(n, seed=0):
    """n map points over the image (octave ratios k + 0.5, view cosines 0.8 or 0.9995) and n keypoints: each map
    point's own near its projection, except that every fifth keypoint is instead a second candidate of the map point
    before it, so later points find keypoints taken.  No margins: for timing."""
    rng = np.random.default_rng(seed)
    T = pose()
    pc = camera_points(rng, n)
    pts = [point_for(rng, T, pc[i], 0.9995 if i % 3 == 0 else 0.8, rng.integers(0, N_SCALES - 1) + 0.5) for i in range(n)]
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    cols = [np.array(c) for c in zip(*pts)]
    r = ref(pack(T, np.zeros((0, 2)), [], np.zeros((0, 32)), [], *cols, desc), np.float64)
    uv2 = r["uv"] + rng.uniform(-0.5, 0.5, (n, 2)) * r["radius"][:, None]
    o2 = r["predicted_octave"].copy()
    d2 = np.stack([ms.flip_bits(desc[i], rng.choice(256, rng.integers(0, 10), replace=False)) for i in range(n)])
    for i in range(4, n, 5):
        uv2[i] = r["uv"][i - 1] + rng.uniform(-0.5, 0.5, 2) * r["radius"][i - 1]
        o2[i] = o2[i - 1]
        d2[i] = ms.flip_bits(desc[i - 1], rng.choice(256, 40, replace=False))
    return pack(T, uv2, o2, d2, np.full(n, -1), *cols, desc)
