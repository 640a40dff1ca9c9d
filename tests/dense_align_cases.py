"""Scenes for the dense aligner's tests (tests/test_dense_align_ref.py and the GPU files): a room corner of three planes that are not
parallel with the sphere of tests/tsdf_cases.py in front of it, so that all six degrees of freedom are held; depth and normals are
rendered analytically on the host from any pose.  The model view is rendered at the identity, the live image at a planted
X = liveInModel.  `class_pair` plants every sample class of the rule into such a pair.  Test infrastructure only."""
import functools

import numpy as np

import tsdf_cases

F = np.float32
CAMERA, ROWS, COLS = tsdf_cases.SPHERE["camera"], tsdf_cases.SPHERE["rows"], tsdf_cases.SPHERE["cols"]
SPHERE = (tsdf_cases.SPHERE["centre"], tsdf_cases.SPHERE["radius"])
# (normal, a point of the plane): a back wall, a floor (y points down) and a left wall, each tilted a little
PLANES = (((0.10, 0.05, -1.0), (0.0, 0.0, 3.0)), ((0.0, -1.0, -0.10), (0.0, 0.8, 2.0)), ((1.0, 0.0, -0.15), (-1.0, 0.0, 2.0)))


def small_camera(rows, cols):
    """a camera of about the field of view of CAMERA for an image of rows x cols pixels"""
    f = 80.0 * cols / 80.0 if cols >= rows else 80.0 * rows / 60.0
    return dict(fx=max(f, 1.0), fy=max(f, 1.0), cx=(cols - 1) / 2.0 + 0.1, cy=(rows - 1) / 2.0 - 0.2)


def offset(t, angles):
    """X [4, 4] float32: a translation t (metres) and rotations (radians) about x, y and z, in this order"""
    ax, ay, az = angles
    cx_, sx, cy_, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    X = np.eye(4)
    X[:3, :3] = Rz @ Ry @ Rx
    X[:3, 3] = t
    return X.astype(F)


def render(pose, camera=CAMERA, rows=ROWS, cols=COLS, sphere=True):
    """the corner seen from pose (camera in the world, [4, 4]) -> (depth [rows, cols] float32 metres of z, 0 = nothing,
    normal [rows, cols, 4] float32 in the camera's frame, towards the camera, fourth float 1 = present)"""
    T = np.asarray(pose, np.float64).reshape(4, 4)
    R, o = T[:3, :3], T[:3, 3]
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    d = np.stack([(u - camera["cx"]) / camera["fx"], (v - camera["cy"]) / camera["fy"], np.ones_like(u, np.float64)], axis=-1)
    dw = d @ R.T
    best = np.full((rows, cols), np.inf)
    normal = np.zeros((rows, cols, 3))
    with np.errstate(all="ignore"):
        for n, point in PLANES:
            n = np.asarray(n, np.float64) / np.linalg.norm(n)
            t = (n @ (np.asarray(point, np.float64) - o)) / (dw @ n)
            hit = (t > 0) & (t < best)
            best = np.where(hit, t, best)
            normal = np.where(hit[..., None], n, normal)
        if sphere:
            c = np.asarray(SPHERE[0], np.float64) - o
            a, b, cc = (dw * dw).sum(-1), -2.0 * (dw @ c), c @ c - SPHERE[1] ** 2
            disc = b * b - 4 * a * cc
            t = (-b - np.sqrt(disc)) / (2 * a)
            hit = (disc > 0) & (t > 0) & (t < best)
            best = np.where(hit, t, best)
            at = o + dw * np.where(hit, t, 0.0)[..., None]
            normal = np.where(hit[..., None], (at - np.asarray(SPHERE[0])) / SPHERE[1], normal)
    seen = np.isfinite(best)
    nc = normal @ R                                            # R^T n per pixel
    nc = np.where(((nc * d).sum(-1) > 0)[..., None], -nc, nc)  # towards the camera
    out = np.zeros((rows, cols, 4), F)
    out[..., :3] = np.where(seen[..., None], nc, 0.0)
    out[..., 3] = seen
    return np.where(seen, best, 0.0).astype(F), out


def to_u16(depth):
    """millimetres"""
    return np.round(np.asarray(depth, np.float64) * 1000.0).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def pair(t=(0.03, -0.02, 0.025), angles=(0.02, -0.03, 0.025), rows=ROWS, cols=COLS, depth_type="f32", camera=None):
    """the model view at the identity and the live image at X = offset(t, angles) -> dict(camera, X_true, model_depth, model_normal,
    live_depth, live_normal, scale).  Shared by the tests: do not write into it"""
    cam = dict(camera) if camera is not None else (CAMERA if (rows, cols) == (ROWS, COLS) else small_camera(rows, cols))
    X = offset(t, angles)
    md, mn = render(np.eye(4), cam, rows, cols)
    ld, ln = render(X, cam, rows, cols)
    out = dict(camera=cam, X_true=X, model_depth=md, model_normal=mn, live_depth=to_u16(ld) if depth_type == "u16" else ld,
               live_normal=ln, scale=1e-3 if depth_type == "u16" else 1.0, depth_type=depth_type)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def class_pair(rows=ROWS, cols=COLS, depth_type="f32", seed=0):
    """a pair at a small offset into which every class is planted: live pixels that are no depths and model pixels without a surface
    or without a normal (unmatched), model depths of +inf and a NaN normal (invalid), a live patch 0.3 m behind the model (the
    distance gate), a live patch whose normals face away (the normal gate), a live patch 0.15 m in front (outliers)"""
    s = {k: (np.array(a) if isinstance(a, np.ndarray) else a)
         for k, a in pair((0.004, -0.003, 0.002), (0.002, -0.001, 0.003), rows, cols, "f32").items()}
    rng = np.random.default_rng([91, rows, cols, seed])
    ld, ln, md, mn = s["live_depth"], s["live_normal"], s["model_depth"], s["model_normal"]

    def patch(k):  # the k-th of six vertical stripes
        return slice(None), slice(k * cols // 6, max((k + 1) * cols // 6, k * cols // 6 + 1))
    some = lambda share: rng.random((rows, cols)) < share  # noqa: E731
    ld[patch(1)] += F(0.3)
    ld[patch(2)] -= F(0.15)
    ln[patch(3)][..., :3] *= F(-1)
    ld[some(0.05)] = 0
    md[some(0.05)] = 0
    mn[some(0.05)] = 0
    md[some(0.03)] = np.inf
    mn[some(0.02), 0] = np.nan
    if depth_type == "u16":
        s["live_depth"], s["scale"], s["depth_type"] = to_u16(ld), 1e-3, "u16"
    else:
        bad = some(0.04)
        ld[bad] = rng.choice(np.array([np.nan, np.inf, -0.0, -1.5], F), int(bad.sum()))
    return s
