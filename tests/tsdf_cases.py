"""Scenes for the TSDF tests (tests/test_tsdf_ref.py and the GPU files): rendered depth images of a sphere and of planes, poses about a
point, random rigid transforms and depth images with steps and values that are not depths.  Test infrastructure only."""
import numpy as np

F = np.float32


def rot_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def pose_about(centre, angle, distance):
    """the camera `distance` from `centre`, rotated by `angle` about the vertical through it and looking at it: [16] float32"""
    R = rot_y(angle)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = np.asarray(centre, np.float64) + R @ np.array([0.0, 0.0, -distance])
    return T.astype(F).reshape(16)


def random_pose(rng, spread=1.0):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3] = q
    T[:3, 3] = rng.uniform(-spread, spread, 3)
    return T.astype(F)


def sphere_depth(pose, camera, rows, cols, centre, radius):
    """the z depth of a sphere seen from pose (camera in the world) [rows, cols] float32, 0 where the ray misses it"""
    T = np.asarray(pose, np.float64).reshape(4, 4)
    c = T[:3, :3].T @ (np.asarray(centre, np.float64) - T[:3, 3])  # the centre in the camera
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    d = np.stack([(u - camera["cx"]) / camera["fx"], (v - camera["cy"]) / camera["fy"], np.ones_like(u, np.float64)], axis=-1)
    a, b, cc = (d * d).sum(-1), -2.0 * (d @ c), c @ c - radius * radius
    disc = b * b - 4 * a * cc
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(disc)) / (2 * a)
    return np.where((disc > 0) & (t > 0), t, 0.0).astype(F)


SPHERE = dict(camera=dict(fx=80.0, fy=80.0, cx=39.5, cy=29.5), rows=60, cols=80, centre=(0.0, 0.0, 2.0), radius=0.5,
              angles=(0.0, 0.5, -0.5, 1.0), voxel_size=0.05, truncation=0.15, dims=(28, 26, 27))


def sphere_scene():
    """the issue's scene: four 80 x 60 views of a sphere of radius 0.5 m at (0, 0, 2), rotated 0, +-0.5 and 1 rad about it, into a
    28 x 26 x 27 volume of 5 cm voxels centred on it -> (seq, origin)"""
    s = SPHERE
    pose = np.stack([pose_about(s["centre"], a, 2.0) for a in s["angles"]])
    depth = np.stack([sphere_depth(p, s["camera"], s["rows"], s["cols"], s["centre"], s["radius"]) for p in pose])
    nx, ny, nz = s["dims"]
    origin = np.array([s["centre"][0] - nx * s["voxel_size"] / 2, s["centre"][1] - ny * s["voxel_size"] / 2,
                       s["centre"][2] - nz * s["voxel_size"] / 2, 0.0], F)
    return dict(depth=depth, pose=pose, n_images=len(pose)), origin


K = dict(fx=30.0, fy=29.0, cx=11.3, cy=9.6)   # the 24 x 20 images of the device cases
ROWS, COLS = 20, 24


def wavy_depth(rng, frames, rows=ROWS, cols=COLS, depth_type="f32", base=1.2, bad=True):
    """depth images of a wavy surface about `base` metres with a step, and (bad) pixels that are not depths: NaN, inf, -0 and negative
    values in f32, 0 in u16 (millimetres)"""
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    out = []
    for f in range(frames):
        d = base + 0.15 * np.sin(0.4 * u + f) + 0.1 * np.cos(0.5 * v - f) + np.where(u > cols * 0.6, 0.5, 0.0)
        d = d + rng.normal(0, 0.01, d.shape)
        if depth_type == "u16":
            d = np.round(d * 1000).astype(np.uint16)
            if bad:
                d[rng.random(d.shape) < 0.08] = 0
        else:
            d = d.astype(F)
            if bad:
                r = rng.random(d.shape)
                d[r < 0.02] = np.nan
                d[(r >= 0.02) & (r < 0.04)] = np.inf
                d[(r >= 0.04) & (r < 0.06)] = -0.0
                d[(r >= 0.06) & (r < 0.08)] = -1.5
                d[(r >= 0.08) & (r < 0.09)] = 0.0
        out.append(d)
    return np.stack(out)
