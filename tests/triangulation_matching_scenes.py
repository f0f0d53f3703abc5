"""TEST INFRASTRUCTURE ONLY: synthetic scenes for searchForTriangulation, the search of fuse and the map edits
of fuse (numpy alone, seeded).

A triangulation-matching scene is a dict with the arguments of Context.search_for_triangulation: uv1 / desc1 /
has1, uv2 / desc2 / has2, kb8, E, th, epipolar_th.

Line scenes are placed by hand.  The camera has no distortion, E = [t]x with t = (1, 0, 0), and every keypoint of
either frame sits in the image column through the principal point, on one of a few "lines" (rows 20 px apart).
There ray2 . (E ray1) = sin(theta1 - theta2): a pair on the same line has error 0, a pair on different lines at
least 0.039 rad, against epipolar_th = 0.01.  Descriptors have their first b bits set, so the distance of two is
the difference of their b.

Cloud scenes are triangulation_scene's two views with planted noisy descriptors.
"""
import numpy as np

from deftri import matching
from deftri.mapmodel import KeyFrame, Map, MapPoint, SE3f, mat_from_quat
from deftri.sim import inv_sigma2_table
import matching_scenes as ms
import projection_scenes as ps
import triangulation_scene as ts

LINE_KB8 = np.array([500.0, 500.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0], np.float32)
LINE_E = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
EPI_TH = 0.01


def pack(uv1, d1, h1, uv2, d2, h2, kb8, E, th=50, epipolar_th=EPI_TH, **extra):
    s = dict(uv1=np.asarray(uv1, np.float32).reshape(-1, 2), desc1=np.asarray(d1, np.uint8).reshape(-1, 32),
             has1=np.asarray(h1, bool).reshape(-1), uv2=np.asarray(uv2, np.float32).reshape(-1, 2),
             desc2=np.asarray(d2, np.uint8).reshape(-1, 32), has2=np.asarray(h2, bool).reshape(-1),
             kb8=np.asarray(kb8, np.float32), E=np.asarray(E, np.float32).reshape(3, 3), th=int(th), epipolar_th=float(epipolar_th))
    s.update(extra)
    return s


def args(s, flag_quirk=True):
    return (s["uv1"], s["desc1"], s["has1"], s["uv2"], s["desc2"], s["has2"], s["kb8"], s["E"], s["th"], s["epipolar_th"],
            flag_quirk)


def ref(s, flag_quirk=True, dtype=np.float32):
    return matching.search_for_triangulation_ref(*args(s, flag_quirk), dtype=dtype)


COUNTERS = ("n1", "n2", "n_matches", "n_occupied", "n_unmatched", "n_stolen", "n_flag_skipped", "flag_row")


def same(got, want):
    """A TriangulationMatchResult against a restatement's dict: every integer output and counter."""
    for k in ("matches", "best_dist", "status"):
        np.testing.assert_array_equal(getattr(got, k), want[k], err_msg=k)
    assert got.n_matches == want["n_matches"]
    for k in COUNTERS:
        assert got.report[k] == want["report"][k], k


def near_threshold(s, r64, rel=1e-3):
    """How many pairs with dist <= 50 the fp64 restatement r64 decides within `rel` of epipolar_th."""
    with np.errstate(invalid="ignore"):
        return int(((r64["dist"] <= 50) & (np.abs(r64["err"] - s["epipolar_th"]) <= rel * s["epipolar_th"])).sum())


def line_scene(rows, keys, th=50, order=None):
    """rows / keys: (line, bits) or (line, bits, has_point) per keypoint of frame 1 / frame 2.  order: a permutation
    of the rows."""
    def frame(spec):
        spec = [tuple(k) + (False,) * (3 - len(k)) for k in spec]
        uv = [[320.0, 260.0 + 20.0 * line] for line, _, _ in spec]      # not the principal point: unproject is 0 / 0 there
        return uv, [ms.first_bits(b) for _, b, _ in spec], [h for _, _, h in spec]
    rows = list(rows) if order is None else [rows[i] for i in order]
    return pack(*frame(rows), *frame(keys), LINE_KB8, LINE_E, th)


CHAIN_D = (48, 44, 40, 36, 32, 28, 24, 20, 16, 12)


def chain_scene(decreasing=True, order=None):
    """Ten rows on line 0 whose distances to keypoint 0 are CHAIN_D (or its reverse) and to keypoint 1 (60 bits more)
    60 - d.  Decreasing: row 0 takes keypoint 1 at 12 and keeps it, every later row takes keypoint 0 from the row
    before it.  Increasing: the same with the keypoints exchanged.  Either way eight rows are robbed and rows 0 and 9
    stay matched.  Keypoint 2 repeats keypoint 0 on another line and is never eligible."""
    d = CHAIN_D if decreasing else CHAIN_D[::-1]
    return line_scene([(0, 10 + k) for k in d], [(0, 10), (0, 70), (3, 10)], th=60, order=order)


def quirk_scene(first_dist, k=5):
    """Row 0 is accepted at distance `first_dist`; then k rows, each alone on its line with its keypoint at distance 4."""
    return line_scene([(0, first_dist)] + [(1 + i, 4) for i in range(k)], [(0, 0)] + [(1 + i, 0) for i in range(k)])


def crowded_row_scene(n_keys=150, seed=0):
    """One row against n_keys keypoints on its line at distances 5 .. 45 (more than 64 pass every test), and a second
    row on another line with one keypoint."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(5, 46, n_keys)
    return line_scene([(0, 0), (2, 0)], [(0, int(b)) for b in bits] + [(2, 7)])


def identical_scene(n):
    """n x n keypoints with one descriptor and E = 0: E ray1 is the zero vector, Eigen's normalized() leaves it, the dot
    product is 0 and the error |pi/2 - acos(0)|: every pair passes."""
    rng = np.random.default_rng(n)
    uv = lambda: np.stack([rng.uniform(100, 600, n), rng.uniform(100, 400, n)], 1)
    z = np.zeros((n, 32), np.uint8)
    return pack(uv(), z, np.zeros(n, bool), uv(), z, np.zeros(n, bool), ts.KB8_1, np.zeros((3, 3)))


def cloud_scene(n1, n2, seed=0, rel=1e-3):
    """triangulation_scene's two views under one calibration: 3/4 of the smaller frame are true pairs whose
    descriptors are a common one with 0 .. 8 bits flipped on either side.  The rest of frame 1 are unrelated
    keypoints; the rest of frame 2 are distractors that carry a true descriptor 12 .. 20 px off its epipolar line,
    and unrelated keypoints.  Every ninth slot of frame 1 and every thirteenth of frame 2 holds a map point; frame 2
    is permuted.  Redrawn until the fp64 restatement decides no pair with dist <= 50 within `rel` of epipolar_th;
    `true2[i]` is the keypoint of frame 2 planted for row i, or -1."""
    n_true = 3 * min(n1, n2) // 4
    for attempt in range(50):
        rng = np.random.default_rng(1000 * seed + attempt)
        uv1, uv2, k1, _, T1w, T2w, _ = ts.scene(n_true, seed=seed + attempt, kb8_2=ts.KB8_1, offsets=False, nans=0)
        base = rng.integers(0, 256, (n_true, 32), dtype=np.uint8)
        noisy = lambda: np.stack([ms.flip_bits(d, rng.choice(256, rng.integers(0, 9), replace=False)) for d in base])
        d1, d2 = noisy(), noisy()
        far = lambda k: np.stack([rng.uniform(150, 600, k), rng.uniform(80, 420, k)], 1)
        m1 = n1 - n_true
        uv1 = np.concatenate([uv1, far(m1)]); d1 = np.concatenate([d1, rng.integers(0, 256, (m1, 32), dtype=np.uint8)])
        m2 = n2 - n_true
        who = rng.integers(0, n_true, m2 // 2)
        off = uv2[who] + np.stack([rng.uniform(-3, 3, len(who)), rng.choice([-1.0, 1.0], len(who)) * rng.uniform(12, 20, len(who))], 1)
        uv2 = np.concatenate([uv2, off, far(m2 - len(who))])
        d2 = np.concatenate([d2, d2[who], rng.integers(0, 256, (m2 - len(who), 32), dtype=np.uint8)])
        perm = rng.permutation(n2)
        true2 = np.full(n1, -1, np.int32)
        true2[:n_true] = np.argsort(perm)[:n_true]
        s = pack(uv1, d1, np.arange(n1) % 9 == 4, uv2[perm], d2[perm], np.arange(n2) % 13 == 6, k1,
                 matching.essential_from_poses(T2w, T1w), true2=true2, attempt=attempt)
        if near_threshold(s, ref(s, False, np.float64), rel) == 0:
            return s
    raise AssertionError("no scene within the margin")


# ---- the search of fuse ---------------------------------------------------------------------------------------
def fuse_args(s):
    return (s["grid"], s["Tcw"], s["kb8"], s["uv2"], s["octave2"], s["desc2"], s["consider"], s["pos"], s["octave"], s["desc"],
            s["th"])


def fuse_ref(s, dtype=np.float32):
    return matching.fuse_search_ref(*fuse_args(s), dtype=dtype)


def fuse_margins_ok(s, r64):
    """projection_scenes.margins_ok's window and cell-rounding margins for the windows of the fp64 restatement r64."""
    n = len(s["pos"])
    probe = dict(r64, view_cos=np.full(n, 0.8), dist=np.ones(n), ratio=np.full(n, np.nan))
    return ps.margins_ok(dict(s, min_dist=np.full(n, 0.5), max_dist=np.full(n, 2.0)), probe)


def fuse_scene(n, seed):
    """n map points over the image at octaves 0 .. 7, a tenth not considered.  Every considered point but each seventh
    gets a keypoint with its descriptor (a few bits flipped) at 0.2 - 0.6 of its radius 2.5 * 1.2^octave, a third of
    them a rival with a near-equal descriptor, a third a keypoint with the exact descriptor outside the window.
    Redrawn whole until the fp64 restatement decides nothing within the margins; every redraw has n points."""
    for attempt in range(200):
        rng = np.random.default_rng(1000 * seed + attempt)
        T = ps.pose()
        pos = ps.to_world(T, ps.camera_points(rng, n))
        octave = rng.integers(0, ps.N_SCALES, n)
        consider = rng.uniform(size=n) >= 0.1
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        s = dict(grid=ps.GRID, Tcw=T, kb8=ps.KB8, uv2=np.zeros((0, 2), np.float32), octave2=np.zeros(0, np.int32),
                 desc2=np.zeros((0, 32), np.uint8), consider=consider, pos=pos.astype(np.float32), octave=octave.astype(np.int32),
                 desc=desc, th=60)
        r = fuse_ref(s, np.float64)
        uv2, o2, d2 = [], [], []
        for i in np.nonzero(consider)[0]:
            if i % 7 == 6:
                continue
            rad, oct_ = float(r["radius"][i]), int(octave[i])
            place = lambda f: r["uv"][i] + f * rad * rng.choice([-1.0, 1.0], 2) * rng.uniform(0.5, 1.0, 2)
            uv2.append(place(rng.uniform(0.2, 0.6))); o2.append(np.clip(oct_ + rng.integers(-1, 2), 0, ps.N_SCALES - 1))
            d2.append(ms.flip_bits(desc[i], rng.choice(256, rng.integers(0, 10), replace=False)))
            if i % 3 == 0:
                uv2.append(place(rng.uniform(0.2, 0.6))); o2.append(oct_)
                d2.append(ms.flip_bits(d2[-1], rng.choice(256, rng.integers(0, 4), replace=False)))
            if i % 3 == 1:
                uv2.append(r["uv"][i] + rng.uniform(1.4, 1.6) * rad * np.array([1.0, 0.3]) * rng.choice([-1.0, 1.0])); o2.append(oct_)
                d2.append(desc[i])
        if not uv2:
            uv2, o2, d2 = [[700.0, 500.0]], [0], [desc[0]]
        perm = rng.permutation(len(uv2))
        s.update(uv2=np.array(uv2, np.float32)[perm], octave2=np.array(o2, np.int32)[perm], desc2=np.array(d2, np.uint8)[perm],
                 attempt=attempt)
        if fuse_margins_ok(s, fuse_ref(s, np.float64)):
            return s
    raise AssertionError("no scene within the margins")


def crowded_fuse_scene():
    """projection_scenes.crowded_scene's three points and 100 keypoints as a fuse search at octave 7 (radius 8.96 px)."""
    c = ps.crowded_scene()
    return dict(grid=c["grid"], Tcw=c["Tcw"], kb8=c["kb8"], uv2=c["uv2"], octave2=c["octave2"], desc2=c["desc2"],
                consider=np.ones(3, bool), pos=c["pos"], octave=np.full(3, 7, np.int32), desc=c["desc"], th=60)


# ---- maps ------------------------------------------------------------------------------------------------------
def _kf(kid, n_slots, rng=None, pose=None, uv=None, desc=None):
    rng = rng or np.random.default_rng(kid)
    return KeyFrame(kid, pose or SE3f(), ts.KB8_1, n_slots, inv_sigma2_table(ps.N_SCALES, ps.FACTOR),
                    keypoints=np.zeros((n_slots, 2), np.float32) if uv is None else uv, octaves=np.zeros(n_slots, np.int32),
                    descriptors=rng.integers(0, 256, (n_slots, 32), dtype=np.uint8) if desc is None else desc)


def observe(m, kf_id, mp, slot):
    m.keyframes[kf_id].map_points[slot] = mp
    m.add_observation(kf_id, mp.id, slot)


def three_keyframe_map():
    """Keyframes 0, 1, 2 with 6 slots each and map points A (id 10: kf0 slot 0, kf1 slot 1), B (id 11: kf1 slot 2,
    kf2 slot 3, kf0 slot 4) and C (id 12: kf2 slot 5): kf0 and kf1 see both A and B."""
    m = Map()
    for k in range(3):
        m.insert_keyframe(_kf(k, 6))
    pts = {pid: MapPoint([0.01 * pid, 0.0, 0.3], pid=pid) for pid in (10, 11, 12)}
    for mp in pts.values():
        m.insert_map_point(mp)
    for kf_id, pid, slot in ((0, 10, 0), (1, 10, 1), (1, 11, 2), (2, 11, 3), (0, 11, 4), (2, 12, 5)):
        observe(m, kf_id, pts[pid], slot)
    return m


def recount_covisibility(m):
    """Map::mCovisibilityGraph_ as a recount from kf_obs: {kf: {other: common points}} without zero entries."""
    out = {}
    for a, oa in m.kf_obs.items():
        for b, ob in m.kf_obs.items():
            c = len(set(oa) & set(ob))
            if a != b and c:
                out.setdefault(a, {})[b] = c
    return out


def check_map(m):
    """The tables agree with each other and with the keyframes' slots; covis is symmetric and equals a recount."""
    for kid, obs in m.kf_obs.items():
        for pid, slot in obs.items():
            assert m.mp_obs[pid][kid] == slot and m.keyframes[kid].map_points[slot] is m.map_points[pid]
    for pid, obs in m.mp_obs.items():
        assert pid in m.map_points
        for kid, slot in obs.items():
            assert m.kf_obs[kid][pid] == slot
    for kid, kf in m.keyframes.items():
        for slot, mp in enumerate(kf.map_points):
            assert mp is None or m.kf_obs[kid].get(mp.id) == slot
    covis = {a: {b: c for b, c in row.items() if c} for a, row in m.covis.items()}
    covis = {a: row for a, row in covis.items() if row}
    assert covis == recount_covisibility(m)
    for a, row in covis.items():
        for b, c in row.items():
            assert covis[b][a] == c


def view_pose(k):
    """Keyframe k of the four-view chain: 0 and 1 are triangulation_scene's pair, 2 and 3 stand between and beside them."""
    T1w, T2w = ts.poses()
    if k < 2:
        return (T1w, T2w)[k]
    q = np.array([[0.001, 0.004, 0.003, 1.0], [-0.003, 0.008, -0.002, 1.0]][k - 2]); q /= np.linalg.norm(q)
    R = mat_from_quat(q).astype(np.float32)
    c = np.array([[0.03, 0.002, -0.015], [0.05, -0.01, -0.03]][k - 2], np.float32)
    return SE3f(R, -(R @ c))


def four_views(n=150, seed=2):
    """Four keyframes without map points that see the same n world points of triangulation_scene, keypoint j of every
    keyframe being point j (0.1 px of noise, the common descriptor with 0 .. 7 bits flipped), all under KB8_1.
    Returns (map, world points)."""
    rng = np.random.default_rng(seed)
    *_, info = ts.scene(n, seed=seed, kb8_2=ts.KB8_1, offsets=False, nans=0)
    world = info["world"]
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    m = Map()
    for k in range(4):
        T = view_pose(k)
        pc = world @ T.R.astype(np.float64).T + T.t.astype(np.float64)
        uv = (ts._project64(ts.KB8_1, pc) + rng.normal(0, 0.1, (n, 2))).astype(np.float32)
        desc = np.stack([ms.flip_bits(d, rng.choice(256, rng.integers(0, 8), replace=False)) for d in base])
        m.insert_keyframe(_kf(k, n, pose=T, uv=uv, desc=desc))
    return m, world


def map_signature(m):
    """What two maps built by the same sequence must share: the tables, the slots and the descriptors."""
    return ({k: dict(v) for k, v in m.kf_obs.items()}, {k: dict(v) for k, v in m.mp_obs.items() if v},
            {k: [None if mp is None else mp.id for mp in kf.map_points] for k, kf in m.keyframes.items()},
            {k: None if mp.descriptor is None else bytes(mp.descriptor) for k, mp in m.map_points.items()})
