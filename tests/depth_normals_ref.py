"""The depth normals' rule (include/proslam_hip_normals.h, "Depth normals") restated in numpy: which pixels are valid, the usable
neighbours, the tangents, the raw normal and its orientation, the gated smoothing window, the counts, the cloud rows and the
per-sequence refusal, in explicit float32 operations in the order the header writes them.  BUILD-DEFINED: the reference has no dense
stage; this file is the specification the kernels are compared with, byte for byte.  Every function takes the scalar type, so the
same rule runs in float64 where a test measures the float32 rule's error.  Test infrastructure only."""
import numpy as np

from depth_cloud_ref import frame_pose, se3_mul

PRS_OK, PRS_ERR_RANGE = 0, -4
F = np.float32
FLT_MAX = np.finfo(np.float32).max


def params(camera, radius=2, smooth=1, max_rel_diff=0.05, range_min=0.1, range_max=10.0, scale=1.0, sensor_in_robot=None, dtype=F):
    S = np.eye(4, dtype=F) if sensor_in_robot is None else np.asarray(sensor_in_robot, F).reshape(4, 4)
    T = dtype
    return dict(fx=T(F(camera["fx"])), fy=T(F(camera["fy"])), cx=T(F(camera["cx"])), cy=T(F(camera["cy"])), range_min=T(F(range_min)),
                range_max=T(F(range_max)), radius=int(radius), smooth=int(smooth), max_rel_diff=T(F(max_rel_diff)), scale=T(F(scale)),
                sensor_in_robot=S.copy(), dtype=dtype)


def shifted(a, dv, du, fill):
    """b[..., v, u] = a[..., v + dv, u + du], and fill where (v + dv, u + du) lies outside the image"""
    rows, cols = a.shape[-2:]
    out = np.full_like(a, fill)
    v0, v1, u0, u1 = max(0, -dv), min(rows, rows - dv), max(0, -du), min(cols, cols - du)
    if v0 < v1 and u0 < u1:
        out[..., v0:v1, u0:u1] = a[..., v0 + dv:v1 + dv, u0 + du:u1 + du]
    return out


def metres(image, p):
    """d = scale * raw where the pixel is valid -- raw > 0 and range_min <= d <= range_max, the dense cloud's test -- and NaN
    elsewhere [rows, cols]"""
    T = p["dtype"]
    raw = np.asarray(image).astype(F).astype(T)  # the element as a float32: a 16-bit value converts exactly
    with np.errstate(all="ignore"):
        d = p["scale"] * raw
        ok = (raw > 0) & (d >= p["range_min"]) & (d <= p["range_max"])
    return np.where(ok, d, T(np.nan))


def _length_ok(len2, T):
    limit = FLT_MAX if T is F else np.finfo(np.float64).max
    with np.errstate(invalid="ignore"):
        return (len2 > 0) & (len2 <= limit)


def raw_normals(d, p):
    """d: metres().  -> (n [3, rows, cols], w [rows, cols], has [rows, cols] bool): the raw normal, zeros where there is none"""
    T = p["dtype"]
    rows, cols = d.shape
    r, nan = p["radius"], T(np.nan)
    with np.errstate(all="ignore"):
        gate = p["max_rel_diff"] * d
        kx = (np.arange(cols).astype(T) - p["cx"]) / p["fx"]
        ky = (np.arange(rows).astype(T) - p["cy"]) / p["fy"]
        P = np.stack([kx[None, :] * d, ky[:, None] * d, d])  # the point of every pixel, NaN at an invalid one
        assert P.dtype == T

        def neighbour(dv, du):
            dq = shifted(d, dv, du, nan)
            return np.abs(dq - d) <= gate, shifted(P, dv, du, nan)  # inside, valid (a NaN compares false) and within the gate

        (ul, PL), (ur, PR), (uu, PU), (ud, PD) = neighbour(0, -r), neighbour(0, r), neighbour(-r, 0), neighbour(r, 0)
        tx = np.where(ur, PR, P) - np.where(ul, PL, P)  # both: R - L; R only: R - c; L only: c - L
        ty = np.where(ud, PD, P) - np.where(uu, PU, P)
        m0 = ty[1] * tx[2] - ty[2] * tx[1]
        m1 = ty[2] * tx[0] - ty[0] * tx[2]
        m2 = ty[0] * tx[1] - ty[1] * tx[0]
        len2 = (m0 * m0 + m1 * m1) + m2 * m2
        has = (ul | ur) & (uu | ud) & _length_ok(len2, T)
        length = np.sqrt(len2)
        n = np.stack([m0 / length, m1 / length, m2 / length])
        dot = (n[0] * P[0] + n[1] * P[1]) + n[2] * P[2]
        n = np.where(dot > 0, -n, n)
    assert n.dtype == T
    w = (ul.astype(np.int32) + ur + uu + ud).astype(T)
    return np.where(has, n, T(0)), np.where(has, w, T(0)), has


def smoothed(d, n, has, p):
    """the raw normals summed over the gated (2 s + 1)^2 window in raster order and renormalised -> (n [3, rows, cols], has)"""
    T = p["dtype"]
    s = p["smooth"]
    with np.errstate(all="ignore"):
        gate = p["max_rel_diff"] * d
        acc = np.zeros_like(n)
        for dv in range(-s, s + 1):
            for du in range(-s, s + 1):
                use = shifted(has, dv, du, False) & (np.abs(shifted(d, dv, du, T(np.nan)) - d) <= gate)
                acc = np.where(use, acc + shifted(n, dv, du, T(0)), acc)
        len2 = (acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]
        keep = has & _length_ok(len2, T)
        out = acc / np.sqrt(len2)
    assert out.dtype == T
    return np.where(keep, out, T(0)), keep


def normals_image(image, p):
    """one depth image [rows, cols] -> normal [rows, cols, 4] in p's scalar type: (n0, n1, n2, w), zeros where there is no normal"""
    T = p["dtype"]
    d = metres(image, p)
    n, w, has = raw_normals(d, p)
    if p["smooth"] > 0:
        n, has = smoothed(d, n, has, p)
        w = np.where(has, w, T(0))
    return np.concatenate([n, w[None]]).transpose(1, 2, 0).astype(T).copy()


def depth_normals(seq, p, before=None, rows=None):
    """seq: one sequence -- depth [frames, rows, cols] (uint16 or float32), n_images (absent or None: frames) and, for the cloud rows,
    pose [pose_stride, 16] float32 and optionally frame_index [frames].  p: params().  before: the output arrays as they stand
    (normal [frames, rows, cols, 4], n_normal [frames], row_normal [row_stride, 4]; None: zeros).  rows: None, or the cloud's rows as
    dict(frame [row_stride], pixel [row_stride], n, base (absent or None: 0)).
    -> dict(status, normal, n_normal and, with rows, row_normal, n_bad_rows (None where a refused sequence leaves it untouched))"""
    depth = np.asarray(seq["depth"])
    frames, nr, nc = depth.shape
    n_img = frames if seq.get("n_images") is None else int(seq["n_images"])
    before = before or {}
    out = dict(normal=np.array(before.get("normal", np.zeros((frames, nr, nc, 4), F)), F, copy=True),
               n_normal=np.array(before.get("n_normal", np.zeros(frames, np.int32)), np.int32, copy=True))
    bad = n_img < 0 or n_img > frames
    if rows is not None:
        stride = len(rows["frame"])
        out["row_normal"] = np.array(before.get("row_normal", np.zeros((stride, 4), F)), F, copy=True)
        out["n_bad_rows"] = None
        base, n = (0 if rows.get("base") is None else int(rows["base"])), int(rows["n"])
        bad = bad or base < 0 or n < 0 or base > stride or n > stride or base > n
    if bad:
        out["status"] = PRS_ERR_RANGE
        return out
    out["status"] = PRS_OK
    for f in range(n_img):
        out["normal"][f] = normals_image(depth[f], p)
        out["n_normal"][f] = int((out["normal"][f][..., 3] > 0).sum())
    if rows is not None:
        n_bad, transforms = 0, {}
        for j in range(base, min(n, stride)):
            f, q = int(rows["frame"][j]), int(rows["pixel"][j])
            pose = None
            if 0 <= f < n_img and 0 <= q < nr * nc:
                _, pose = frame_pose(seq, f)
            if pose is None:
                out["row_normal"][j] = 0
                n_bad += 1
                continue
            if f not in transforms:
                transforms[f] = se3_mul(pose, p["sensor_in_robot"])
            T = transforms[f]
            n = out["normal"][f].reshape(-1, 4)[q]
            with np.errstate(all="ignore"):
                for i in range(3):
                    out["row_normal"][j, i] = F(F(F(T[i, 0] * n[0]) + F(T[i, 1] * n[1])) + F(T[i, 2] * n[2]))
            out["row_normal"][j, 3] = n[3]
        out["n_bad_rows"] = n_bad
    return out


def angle_between(a, b):
    """the angle in radians between unit vectors [..., 3], in float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1))
