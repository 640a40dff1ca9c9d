"""The dense RGB-D cloud's rule (include/proslam_hip.h, "Dense RGB-D cloud") restated in numpy for one sequence: which frames are
skipped, which pixels are kept, the point of a pixel in explicit float32 operations in the order of prs_se3.h's se3_mul / se3_apply,
the order of the rows, n_base, truncation, the count-only call and the per-sequence refusal.  BUILD-DEFINED: the reference's
unprojector lies outside its tree; this file is what the kernels are compared with, byte for byte.  Test infrastructure only."""
import numpy as np

PRS_OK, PRS_ERR_CAPACITY, PRS_ERR_RANGE = 0, -2, -4
F = np.float32
INT32_MAX = (1 << 31) - 1


def params(camera, range_min=0.1, range_max=10.0, step=1, scale=1.0, sensor_in_robot=None):
    S = np.eye(4, dtype=F) if sensor_in_robot is None else np.asarray(sensor_in_robot, F).reshape(4, 4)
    return dict(fx=F(camera["fx"]), fy=F(camera["fy"]), cx=F(camera["cx"]), cy=F(camera["cy"]), range_min=F(range_min),
                range_max=F(range_max), step=int(step), scale=F(scale), sensor_in_robot=S.copy())


def se3_mul(A, B):
    """prs_se3.h se3_mul on float32 [4, 4]: the top three rows, (a0 b0 + a1 b1) + a2 b2 and, in the last column, + a3"""
    A, B = np.asarray(A, F).reshape(4, 4), np.asarray(B, F).reshape(4, 4)
    T = np.zeros((4, 4), F)
    T[3, 3] = F(1)
    for i in range(3):
        for j in range(3):
            T[i, j] = F(F(F(A[i, 0] * B[0, j]) + F(A[i, 1] * B[1, j])) + F(A[i, 2] * B[2, j]))
        T[i, 3] = F(F(F(F(A[i, 0] * B[0, 3]) + F(A[i, 1] * B[1, 3])) + F(A[i, 2] * B[2, 3])) + A[i, 3])
    return T


def se3_apply(T, p):
    """prs_se3.h se3_apply on float32 points [n, 3]: ((t0 p0 + t1 p1) + t2 p2) + t3 per row of T"""
    T, p = np.asarray(T, F), np.asarray(p, F)
    out = np.zeros((p.shape[0], 3), F)
    for i in range(3):
        out[:, i] = ((T[i, 0] * p[:, 0] + T[i, 1] * p[:, 1]) + T[i, 2] * p[:, 2]) + T[i, 3]
    return out


def frame_pose(seq, f):
    """the pose row k of image f and its [4, 4] float32 pose, or (k, None) when the frame is skipped"""
    pose = np.asarray(seq["pose"], F).reshape(-1, 16)
    k = int(seq["frame_index"][f]) if seq.get("frame_index") is not None else f
    if k < 0 or k >= pose.shape[0] or not np.isfinite(pose[k, :12]).all():
        return k, None
    return k, pose[k].reshape(4, 4)


def unproject(image, p, gray=None):
    """one image -> (points in the camera [n, 3] float32, intensity [n] float32, pixel [n] int32): the sampled pixels that pass the
    depth test, in raster order"""
    image = np.asarray(image)
    rows, cols = image.shape
    step = p["step"]
    v, u = np.meshgrid(np.arange(0, rows, step), np.arange(0, cols, step), indexing="ij")
    v, u = v.reshape(-1), u.reshape(-1)
    raw = image[v, u].astype(F)  # a 16-bit value converts exactly
    with np.errstate(all="ignore"):
        d = p["scale"] * raw
        keep = (raw > F(0)) & (d >= p["range_min"]) & (d <= p["range_max"])
        u, v, d = u[keep], v[keep], d[keep]
        x = (u.astype(F) - p["cx"]) / p["fx"] * d
        y = (v.astype(F) - p["cy"]) / p["fy"] * d
    pts = np.stack([x, y, d], axis=1).astype(F)
    assert x.dtype == F and y.dtype == F and d.dtype == F
    if gray is None:
        inten = np.zeros(u.size, F)
    else:
        inten = np.asarray(gray)[v, u].astype(F) * (F(1.0) / F(255.0))
    return pts, inten, (v * cols + u).astype(np.int32)


def depth_cloud(seq, p, out_stride, before=None, count_only=False):
    """seq: one sequence -- depth [frames, rows, cols] (uint16 or float32), n_images, pose [pose_stride, 16] float32 and optionally
    frame_index [frames], gray [frames, rows, cols] uint8, n_base (absent or None: not set).  p: params().  before: the output arrays
    as they stand (dict of xyz [out_stride, 4], frame, pixel [out_stride]; None: zeros), which the call changes in rows n_base ..
    n_out - 1 alone.
    -> dict(status, n_out, n_total, n_skipped, xyz, frame, pixel): the whole output arrays after the call"""
    depth = np.asarray(seq["depth"])
    frames, n_img = depth.shape[0], int(seq["n_images"])
    cap = max(int(out_stride), 0)
    base = int(seq["n_base"]) if seq.get("n_base") is not None else 0
    before = before or {}
    out = dict(xyz=np.array(before.get("xyz", np.zeros((cap, 4), F)), F, copy=True),
               frame=np.array(before.get("frame", np.zeros(cap, np.int32)), np.int32, copy=True),
               pixel=np.array(before.get("pixel", np.zeros(cap, np.int32)), np.int32, copy=True))
    if n_img < 0 or n_img > frames or base < 0 or base > cap:
        out.update(status=PRS_ERR_RANGE, n_total=0, n_skipped=0, n_out=min(max(base, 0), cap))
        return out
    xyz, frame, pixel, skipped = [], [], [], 0
    for f in range(n_img):
        _, pose = frame_pose(seq, f)
        if pose is None:
            skipped += 1
            continue
        T = se3_mul(pose, p["sensor_in_robot"])
        gray = seq["gray"][f] if seq.get("gray") is not None else None
        pts, inten, pix = unproject(depth[f], p, gray)
        with np.errstate(all="ignore"):
            w = se3_apply(T, pts)
        xyz.append(np.concatenate([w, inten[:, None]], axis=1).astype(F))
        frame.append(np.full(pix.size, f, np.int32))
        pixel.append(pix)
    kept = sum(x.shape[0] for x in xyz)
    total = min(base + kept, INT32_MAX)
    out.update(n_total=total, n_skipped=skipped)
    if count_only:
        out.update(status=PRS_OK, n_out=base)
        return out
    n_out = min(total, cap)
    out.update(status=PRS_ERR_CAPACITY if total > cap else PRS_OK, n_out=n_out)
    if kept:
        m = n_out - base
        out["xyz"][base:n_out] = np.concatenate(xyz)[:m]
        out["frame"][base:n_out] = np.concatenate(frame)[:m]
        out["pixel"][base:n_out] = np.concatenate(pixel)[:m]
    return out


def host_route(depth, pose, p):
    """the route the device call replaces, for tools/bench_depth_cloud.py: host depth images [frames, rows, cols] and poses
    [frames, 16] through numpy -> xyz [n, 4]"""
    seq = dict(depth=depth, n_images=depth.shape[0], pose=pose)
    s = p["step"]
    out = depth_cloud(seq, p, depth.shape[0] * len(range(0, depth.shape[1], s)) * len(range(0, depth.shape[2], s)))
    return out["xyz"][:out["n_out"]]
