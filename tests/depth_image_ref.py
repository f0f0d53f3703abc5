"""TEST INFRASTRUCTURE ONLY: numpy restatement of the reference's real-image depth path.

  sample()          KeyFrame::getDepthMeasure(x, y, scaled) (KeyFrame.cc:181-202) over Interpolate
                    (Geometry.cc:607-620), every operation rounded to float32 in the reference's order,
                    with the per-pixel status of include/deftri.h.
  real_absolute()   measureRealAbsoluteMapErrors (Measurements.cc:101-348); `accumulate` chooses the
                    reference's sequential float32 accumulation or fp64 fixed-tree sums of the same terms.
  relative()        measureRelativeMapErrors (:350-518) with the depths from the images, including the
                    reference's lookup of keyframe 1's keypoint idx2 in keyframe 2's image (:432,440).
  synthetic_images() depth images in which every keypoint's lookup is near its simulated depth.
"""
import numpy as np

from oracle import graph_ref

f32 = np.float32


def sample(img, uv, image_depth_scale=1.0, scaled=True):
    """(depth float64 [n], status uint8 [n]); depth is NaN where status != 0."""
    img = np.ascontiguousarray(img, f32)
    rows, cols = img.shape
    flat = img.reshape(-1)
    uv = np.asarray(uv, f32).reshape(-1, 2)
    depth = np.full(len(uv), np.nan)
    status = np.zeros(len(uv), np.uint8)
    one = f32(1)
    for k, (x, y) in enumerate(uv):
        if x >= cols or y >= rows:                    # the reference's out_of_range test comes first
            status[k] = 1
            continue
        if not (x >= 0) or not (y >= 0):              # negative or NaN ((int) of it / a read before the buffer)
            status[k] = 2
            continue
        x_, y_ = f32(np.trunc(x)), f32(np.trunc(y))
        r, c = int(y_), int(x_)
        if (r + 1) * cols + c + 1 >= rows * cols:      # the last of the four linear indices
            status[k] = 2
            continue
        _x, _y = f32(x - x_), f32(y - y_)             # modf's fractional part is exact
        w00 = f32(f32(one - _x) * f32(one - _y))
        w01 = f32(f32(one - _x) * _y)
        w10 = f32(_x * f32(one - _y))
        w11 = f32(f32(f32(one - w00) - w01) - w10)
        g = f32(f32(f32(f32(flat[r * cols + c] * w00) + f32(flat[r * cols + c + 1] * w10)) +
                    f32(flat[(r + 1) * cols + c] * w01)) + f32(flat[(r + 1) * cols + c + 1] * w11))
        d = float(g) / 100
        depth[k] = d if scaled else d * float(image_depth_scale)
    return depth, status


def synthetic_images(m, shape, seed, image_depth_scale=None, ph=None):
    """Give every keyframe of `m` a depth image (rows, cols) = shape: a noisy background at the median
    depth, then the four pixels around every keypoint set to that keypoint's simulated depth (x 100 /
    scale), so each lookup is near the simulated depth."""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    for n, kf in enumerate(m.keyframes.values()):
        scale = (1.0 + 0.25 * n) if image_depth_scale is None else image_depth_scale
        img = (np.median(kf.depth) * 100 / scale * (1 + 0.01 * rng.standard_normal((rows, cols)))).astype(f32)
        for (x, y), d in zip(kf.keypoints, kf.depth):
            r, c = int(y), int(x)
            if 0 <= r < rows - 1 and 0 <= c < cols - 1:
                img[r:r + 2, c:c + 2] = f32(d * 100 / scale)
        k = kf.kb8
        kf.set_depth_image(img, scale, [k[0], k[1], k[2], k[3]] if ph is None else ph)
    return m


def keyframe_depths(kf, scaled):
    """getDepthMeasure of every keypoint of a keyframe from its own image."""
    return sample(kf.depth_image, kf.keypoints, kf.image_depth_scale, scaled)


_TAG = 4096


def tagged(m):
    """A copy of `m` without images whose per-index depths name their row: depth[j] = j + 4096 * kf id
    (exact in float32), so a per-index graph build's dep_meas identifies every depth edge."""
    import copy
    t = copy.deepcopy(m)
    for kf in t.keyframes.values():
        kf.set_depth_image(None)
        kf.depth = (np.arange(len(kf.keypoints)) + _TAG * kf.id).astype(f32)
    return t


def dep_meas_from_tags(m, tags):
    """The restated dep_meas of `m` (getDepthMeasure(u, v, false) for keyframes with an image, the
    per-index depth otherwise) for the depth edges a tagged build names."""
    per_kf = {}
    for kf in m.keyframes.values():
        per_kf[kf.id] = keyframe_depths(kf, False)[0] if kf.depth_image is not None else kf.depth.astype(np.float64)
    tags = np.asarray(tags).astype(np.int64)
    return np.array([per_kf[int(t) // _TAG][int(t) % _TAG] for t in tags])


# ---- measureRealAbsoluteMapErrors --------------------------------------------------------------

def _quat_f32(kf):
    a = kf.pose.as7()
    return np.asarray(a[:4]).astype(f32), np.asarray(a[4:]).astype(f32)


def _rot_f32(q):
    x, y, z, w = (f32(v) for v in q)
    two, one = f32(2), f32(1)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], f32)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def _qrot(q, v):
    """Eigen QuaternionBase::_transformVector in float32."""
    uv = _cross(q[:3], v)
    uv = uv + uv
    return (v + q[3] * uv) + _cross(q[:3], uv)


def _inverse_rows(q, t):
    """Sophus SE3f::inverse().matrix(): R of the conjugate, invR * (-t)."""
    qi = np.array([-q[0], -q[1], -q[2], q[3]], f32)
    return _rot_f32(qi), _qrot(qi, -t)


def _h(R, t, x):
    """4x4 * [x; 1] column by column (Eigen's lazy product), float32."""
    return np.array([((R[r, 0] * x[0] + R[r, 1] * x[1]) + R[r, 2] * x[2]) + t[r] for r in range(3)], f32)


def _sqn(v):
    return f32(f32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _tree_sum(v):
    """A fixed pairwise fp64 sum (one legal fixed-order tree)."""
    v = np.asarray(v, np.float64)
    if len(v) == 0:
        return 0.0
    while len(v) > 1:
        if len(v) % 2:
            v = np.append(v, 0.0)
        v = v[0::2] + v[1::2]
    return float(v[0])


def real_absolute(m, accumulate="f32"):
    """accumulate "f32": the reference's sequential float accumulators; "f64": every sum an fp64 fixed
    tree over the pair's terms, cast to float where the reference's accumulator is read."""
    order = m.kf_order()
    point_count = len(m.map_points)
    tm = te = tsq = tup = f32(0) if accumulate == "f32" else 0.0
    scale1 = scale2 = f32(0)
    n_points = 0
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            kf1, kf2 = m.keyframes[order[b]], m.keyframes[order[a]]
            ph = kf1.ph.astype(f32)
            q1, t1 = _quat_f32(kf1); q2, t2 = _quat_f32(kf2)
            Ri1, ti1 = _inverse_rows(q1, t1); Ri2, ti2 = _inverse_rows(q2, t2)
            dd1, st1 = keyframe_depths(kf1, True); dd2, st2 = keyframe_depths(kf2, True)
            rows = []
            for i in range(kf1.n_slots):
                mp1, mp2 = kf1.map_points[i], kf2.map_points[i]
                if mp1 is None or mp2 is None:
                    continue
                i1 = m.is_map_point_in_keyframe(mp1.id, kf1.id); i2 = m.is_map_point_in_keyframe(mp2.id, kf2.id)
                if i1 < 0 or i2 < 0:
                    continue
                assert st1[i1] == 0 and st2[i2] == 0
                rows.append((kf1.keypoints[i1].astype(f32), kf2.keypoints[i2].astype(f32), f32(dd1[i1]), f32(dd2[i2]),
                             mp1.position.astype(f32), mp2.position.astype(f32)))
            unp = lambda x: np.array([(x[0] - ph[2]) / ph[0], (x[1] - ph[3]) / ph[1], f32(1)], f32)
            mov, e1s, e2s, s1s, s2s, r1, r2 = [], [], [], [], [], [], []
            for x1, x2, d1, d2, p1, p2 in rows:
                m1 = unp(x1); m1 = m1 / m1[2]; x3d1 = m1 * d1
                m2 = unp(x2); m2 = m2 / m2[2]; x3d2 = m2 * d2
                w1, w2 = _h(Ri1, ti1, x3d1), _h(Ri2, ti2, x3d2)
                c1 = _qrot(q1, p1) + t1; c2 = _qrot(q2, p2) + t2
                r1.append(f32(x3d1[2] / c1[2])); r2.append(f32(x3d2[2] / c2[2]))
                mov.append(np.sqrt(_sqn(w1 - w2)))
                s1, s2 = _sqn(p1 - w1), _sqn(p2 - w2)
                e1s.append(np.sqrt(s1)); e2s.append(np.sqrt(s2)); s1s.append(s1); s2s.append(s2)
            n_points += len(rows)
            if accumulate == "f32":
                for k in range(len(rows)):
                    tm = f32(tm + mov[k]); te = f32(te + f32(e2s[k] + e1s[k])); tsq = f32(tsq + f32(s1s[k] + s2s[k]))
                    scale1 = f32(scale1 + r1[k]); scale2 = f32(scale2 + r2[k])
            else:
                tm += _tree_sum(mov); te += _tree_sum(e1s) + _tree_sum(e2s); tsq += _tree_sum(s1s) + _tree_sum(s2s)
                scale1 = f32(float(scale1) + _tree_sum(r1)); scale2 = f32(float(scale2) + _tree_sum(r2))
            with np.errstate(invalid="ignore", divide="ignore"):
                scale1 = f32(scale1 / f32(n_points)); scale2 = f32(scale2 / f32(n_points))
            u1, u2 = [], []
            for x1, x2, d1, d2, p1, p2 in rows:
                m1 = unp(x1); m1 = m1 / m1[2]; x3d1 = (m1 * d1) / scale1
                m2 = unp(x2); m2 = m2 / m2[2]; x3d2 = (m2 * d2) / scale2
                u1.append(np.sqrt(_sqn(p1 - _h(Ri1, ti1, x3d1)))); u2.append(np.sqrt(_sqn(p2 - _h(Ri2, ti2, x3d2))))
            if accumulate == "f32":
                for k in range(len(rows)):
                    tup = f32(tup + f32(u2[k] + u1[k]))
            else:
                tup += _tree_sum(u1) + _tree_sum(u2)
    out = {"point_count": point_count, "n_points": n_points, "scale1": float(scale1), "scale2": float(scale2),
           "in_kf": int(point_count / 2.0),
           "average_movement": 0.0, "average_error": 0.0, "rmse": 0.0, "average_up_to_scale_error": 0.0}
    if point_count > 0:
        tm, te, tsq, tup = f32(tm), f32(te), f32(tsq), f32(tup)
        out["average_movement"] = float(f32(tm / f32(out["in_kf"]))) * 1000
        out["average_error"] = float(f32(te / f32(point_count))) * 1000
        out["rmse"] = float(np.sqrt(f32(tsq / f32(point_count)))) * 1000
        out["average_up_to_scale_error"] = float(f32(tup / f32(point_count))) * 1000
    return out


# ---- measureRelativeMapErrors with images ------------------------------------------------------

def relative(m):
    """tests/measurements_ref.relative with d1 = kf1.getDepthMeasure(kf1 keypoint idx1, false) and d2 =
    kf2.getDepthMeasure(kf1 keypoint idx2, false) for keyframes that have an image."""
    from measurements_ref import _R_f32
    order = m.kf_order()
    depth = glob = meansq = 0.0
    valid = matches = 0
    out = []
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            kf1, kf2 = m.keyframes[order[b]], m.keyframes[order[a]]
            T = m.get_global_T(kf1.id, kf2.id)
            Rg = _R_f32(T).astype(np.float64); Ts = T.t.astype(f32).astype(np.float64)
            s1, s2 = kf1.estimated_depth_scale, kf2.estimated_depth_scale
            v1 = np.array([mp.position.astype(np.float64) for mp in kf1.map_points if mp is not None])
            v2 = np.array([mp.position.astype(np.float64) for mp in kf2.map_points if mp is not None])
            tri, _ = graph_ref.delaunay_mesh(v1)
            adj, _, area = graph_ref.mesh_structures(v1, tri)
            pos_idx = graph_ref.create_vector_map(v1)
            inv = {int(pos_idx[v]): v for v in range(len(v1))}
            cams = []
            for kf in (kf1, kf2):
                q = kf.pose.as7()[:4]; q = q / np.linalg.norm(q)
                cams.append((graph_ref._mat_from_quat(q), kf.pose.as7()[4:]))
            for i in range(min(kf1.n_slots, kf2.n_slots)):
                mp1, mp2 = kf1.map_points[i], kf2.map_points[i]
                if mp1 is None or mp2 is None:
                    continue
                i1 = m.is_map_point_in_keyframe(mp1.id, kf1.id); i2 = m.is_map_point_in_keyframe(mp2.id, kf2.id)
                if i1 < 0 or i2 < 0:
                    continue
                if kf1.depth_image is not None:
                    (d1,), (st,) = sample(kf1.depth_image, kf1.keypoints[i1], kf1.image_depth_scale, False)
                    assert st == 0
                else:
                    d1 = float(kf1.depth[i1])
                if kf2.depth_image is not None:
                    (d2,), (st,) = sample(kf2.depth_image, kf1.keypoints[i2], kf2.image_depth_scale, False)
                    assert st == 0
                else:
                    d2 = float(kf2.depth[i2])
                for (R, t), mp, d, s in ((cams[0], mp1, d1, s1), (cams[1], mp2, d2, s2)):
                    zc = (R @ mp.position.astype(np.float64) + t)[2]
                    depth += (float(d) - zc * s) ** 2
                if i >= len(v1) or i not in inv or not adj[inv[i]]:
                    continue
                for j in sorted(adj[inv[i]]):
                    pj = int(pos_idx[j])
                    if i >= len(v2) or pj >= len(v2):
                        continue
                    d1v = v1[i] - v1[pj]; d2v = v2[i] - v2[pj]
                    meansq += float(((d2v - d1v) ** 2).sum())
                    valid += 1
                    g = ((Rg @ v2[i] - Ts) - v1[i]) + ((Rg @ v2[pj] - Ts) - v1[pj])
                    glob += float((g * g).sum())
                matches += 1
            out.append({"kf1": kf1.id, "kf2": kf2.id, "reported": int(valid > 1), "rel_error": meansq / area,
                        "depth_error": depth, "global_t_error": glob / area, "area": area, "valid_pairs": valid,
                        "n_matches": matches})
    return out
