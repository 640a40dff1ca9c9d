"""The depth consistency filter's rule (include/proslam_hip.h, "Depth consistency filter") restated in numpy for one sequence: which
frames are usable, the camera poses in float32 (depth_cloud_ref.se3_mul: the dense cloud's order), the relative transform in float64
rounded to float32, the validity test, the votes of the neighbours in explicit float32 operations, the decision and the counts.
BUILD-DEFINED: the reference has no dense images; this file is what the kernels are compared with, byte for byte.  Test
infrastructure only."""
import numpy as np

import depth_cloud_ref as cloud

PRS_OK, PRS_ERR_RANGE = 0, -4
F = np.float32
D = np.float64


def params(camera, window=2, stride=1, max_rel_diff=0.02, min_support=2, max_violation=1, range_min=0.1, range_max=10.0, scale=1.0,
           sensor_in_robot=None):
    p = cloud.params(camera, range_min, range_max, 1, scale, sensor_in_robot)
    p.update(window=int(window), stride=int(stride), max_rel_diff=F(max_rel_diff), min_support=int(min_support),
             max_violation=int(max_violation))
    return p


def camera_pose(seq, f, p):
    """C_f = se3_mul(pose[k], sensor_in_robot) [4, 4] float32, or None when the frame is not usable"""
    _, pose = cloud.frame_pose(seq, f)
    return None if pose is None else cloud.se3_mul(pose, p["sensor_in_robot"])


def relative(Cf, Cg):
    """M = C_g^-1 C_f, the top three rows [3, 4] float32: float64 from the float32 poses, the translations subtracted first"""
    Cf, Cg = np.asarray(Cf, F), np.asarray(Cg, F)
    Rf, Rg = Cf[:3, :3].astype(D), Cg[:3, :3].astype(D)
    dt = Cf[:3, 3].astype(D) - Cg[:3, 3].astype(D)
    M = np.zeros((3, 4), D)
    for i in range(3):
        for j in range(3):
            M[i, j] = (Rg[0, i] * Rf[0, j] + Rg[1, i] * Rf[1, j]) + Rg[2, i] * Rf[2, j]
        M[i, 3] = (Rg[0, i] * dt[0] + Rg[1, i] * dt[1]) + Rg[2, i] * dt[2]
    with np.errstate(over="ignore"):  # a baseline beyond float32 becomes inf, as the device's conversion makes it
        return M.astype(F)


def valid(image, p):
    """(valid [rows, cols] bool, d [rows, cols] float32 the scaled depth) of every element of an image"""
    raw = np.asarray(image).astype(F)  # a 16-bit value converts exactly
    with np.errstate(all="ignore"):
        d = p["scale"] * raw
        ok = (raw > F(0)) & (d >= p["range_min"]) & (d <= p["range_max"])
    assert d.dtype == F
    return ok, d


def votes(image, neighbour, M, p):
    """(support, violation) [rows, cols] bool: the vote of one existing slot for every pixel of image"""
    rows, cols = image.shape
    ok, d = valid(image, p)
    ok_g, d_g = valid(neighbour, p)
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    with np.errstate(all="ignore"):
        p0 = (u.astype(F) - p["cx"]) / p["fx"] * d
        p1 = (v.astype(F) - p["cy"]) / p["fy"] * d
        q = [((M[i, 0] * p0 + M[i, 1] * p1) + M[i, 2] * d) + M[i, 3] for i in range(3)]
        assert all(c.dtype == F for c in q)
        x = np.floor((q[0] / q[2] * p["fx"] + p["cx"]) + F(0.5))
        y = np.floor((q[1] / q[2] * p["fy"] + p["cy"]) + F(0.5))
        assert x.dtype == F and y.dtype == F
        inside = ok & (q[2] > F(0)) & (x >= F(0)) & (x < F(cols)) & (y >= F(0)) & (y < F(rows))
        xi, yi = np.where(inside, x, F(0)).astype(np.int64), np.where(inside, y, F(0)).astype(np.int64)
        voting = inside & ok_g[yi, xi]
        e = d_g[yi, xi] - q[2]
        tol = p["max_rel_diff"] * q[2]
        assert e.dtype == F and tol.dtype == F
        support = voting & (e >= -tol) & (e <= tol)
        violation = voting & (e > tol)
    return support, violation


def slots_of(f, p):
    """the neighbour frames of f, whether they exist or not"""
    js = range(1, p["window"] + 1)
    return [f - j * p["stride"] for j in js] + [f + j * p["stride"] for j in js]


def depth_consistency(seq, p):
    """seq: one sequence -- depth [frames, rows, cols] (uint16 or float32), pose [pose_stride, 16] float32 and optionally n_images
    (absent or None: frames), frame_index [frames].  p: params().
    -> dict(status, n_skipped, results): results[f] = None for an image the call does not touch, else dict(out, support, violation,
    n_kept, n_removed); n_skipped is None when the sequence is refused after n_skipped = 0 was written (it is 0 then)"""
    depth = np.asarray(seq["depth"])
    frames = depth.shape[0]
    n_img = frames if seq.get("n_images") is None else int(seq["n_images"])
    if n_img < 0 or n_img > frames:
        return dict(status=PRS_ERR_RANGE, n_skipped=0, results=[None] * frames)
    C = [camera_pose(seq, f, p) for f in range(n_img)]
    results, skipped = [None] * frames, 0
    for f in range(n_img):
        ok, _ = valid(depth[f], p)
        support, violation = np.zeros(depth[f].shape, np.uint8), np.zeros(depth[f].shape, np.uint8)
        if C[f] is None:
            skipped += 1
            results[f] = dict(out=np.zeros_like(depth[f]), support=support, violation=violation, n_kept=0, n_removed=int(ok.sum()))
            continue
        for g in slots_of(f, p):
            if 0 <= g < n_img and C[g] is not None:
                s, w = votes(depth[f], depth[g], relative(C[f], C[g]), p)
                support += s.astype(np.uint8)
                violation += w.astype(np.uint8)
        keep = ok & (support >= p["min_support"]) & (violation <= p["max_violation"])
        out = np.where(keep, depth[f], depth.dtype.type(0)).astype(depth.dtype)
        results[f] = dict(out=out, support=support, violation=violation, n_kept=int(keep.sum()), n_removed=int((ok & ~keep).sum()))
    return dict(status=PRS_OK, n_skipped=skipped, results=results)


# ---- the synthetic scene of the tests and of tools/bench_depth_consistency.py ----------------------------------------------------------
SCENE_CAMERA = dict(fx=60.0, fy=60.0, cx=31.5, cy=23.5)
SCENE_ROWS, SCENE_COLS, SCENE_FRAMES = 48, 64, 5


def yaw_pose(theta, t):
    """[16] float32: the rotation by theta about y, at t"""
    c, s = np.cos(theta), np.sin(theta)
    T = np.eye(4)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = t
    return T.astype(F).reshape(16)


def scene_poses(frames=SCENE_FRAMES):
    """camera i at (0.15 (i - 2), 0.01 i, 0.05 i), yawed by 0.02 (i - 2)"""
    return np.stack([yaw_pose(0.02 * (i - 2), (0.15 * (i - 2), 0.01 * i, 0.05 * i)) for i in range(frames)])


def scene_depth(pose, rows=SCENE_ROWS, cols=SCENE_COLS, camera=SCENE_CAMERA):
    """the depth image [rows, cols] float32 of the scene from a camera pose [16], by analytic ray casting in float64: the plane
    z = 5 with the rectangle |x| <= 0.6, |y| <= 0.4 at z = 3 in front of it.  The depth along the camera's axis is the ray
    parameter, the ray's camera z being 1"""
    T = np.asarray(pose, D).reshape(4, 4)
    v, u = np.meshgrid(np.arange(rows, dtype=D), np.arange(cols, dtype=D), indexing="ij")
    ray = np.stack([(u - camera["cx"]) / camera["fx"], (v - camera["cy"]) / camera["fy"], np.ones_like(u)], axis=-1) @ T[:3, :3].T
    near = (3.0 - T[2, 3]) / ray[..., 2]
    hit = T[:3, 3] + near[..., None] * ray
    far = (5.0 - T[2, 3]) / ray[..., 2]
    on_rectangle = (np.abs(hit[..., 0]) <= 0.6) & (np.abs(hit[..., 1]) <= 0.4)
    return np.where(on_rectangle, near, far).astype(F)


def scene(seed=7, fraction=0.05):
    """(seq, planted [frames, rows, cols] bool): five views of the scene with `fraction` of the pixels' depths multiplied by a factor
    in [0.5, 0.8] or [1.25, 2]"""
    rng = np.random.default_rng(seed)
    pose = scene_poses()
    depth = np.stack([scene_depth(T) for T in pose])
    planted = rng.random(depth.shape) < fraction
    factor = np.where(rng.random(depth.shape) < 0.5, rng.uniform(0.5, 0.8, depth.shape), rng.uniform(1.25, 2.0, depth.shape))
    depth = np.where(planted, depth * factor, depth).astype(F)
    return dict(depth=depth, pose=pose), planted
