"""Scenes and truth for the dense tracker's loop tests (tests/test_dense_loop_ref.py, tests/test_dense_loop_gpu.py): the corner and
sphere of tests/dense_align_cases.py seen along two trajectories of eight frames, in a world frame G that is a quarter turn and a
translation away from the scene's own, so that every pose the tracker holds is a real world pose and the side on which it composes X
shows.  A quarter turn about y keeps the volume's box aligned with the axes.  `scene_distance` is the truth the fused map is held to.
Test infrastructure only."""
import functools

import numpy as np

import dense_align_cases as cases

CAMERA, ROWS, COLS = cases.CAMERA, cases.ROWS, cases.COLS
VS, TRUNCATION = 0.04, 0.16
# world = G * local: x_world = z + 4, y_world = y - 2, z_world = -x + 7
G = np.array([[0.0, 0.0, 1.0, 4.0], [0.0, 1.0, 0.0, -2.0], [-1.0, 0.0, 0.0, 7.0], [0.0, 0.0, 0.0, 1.0]])
# the box of tests/test_dense_align_gpu.py (70 x 55 x 60 voxels of 4 cm from (-1.4, -1.1, 1.1)) through G
DIMS, ORIGIN = (60, 55, 70), (5.1, -3.1, 5.6, 0.0)
FRAMES = 8
# name -> (start, increment D), each (translation in metres, rotations in radians); local[k] = local[k - 1] * D
TRAJECTORIES = {"A": (((0.1, 0.02, -0.05), (0.03, -0.08, 0.04)), ((0.02, -0.012, 0.015), (0.012, -0.015, 0.01))),
                "B": (((-0.12, 0.03, 0.04), (-0.02, 0.07, -0.03)), ((-0.015, 0.01, -0.02), (-0.01, 0.012, 0.015)))}
EMPTY = {"A": (), "B": (3,)}      # the frames that are all zeros: nothing to align, nothing to fuse
DEPTH_TYPES = ("f32", "u16")
SCALE = {"f32": 1.0, "u16": 1e-3}


@functools.lru_cache(maxsize=None)
def local_poses(name):
    """the camera in the scene's frame at every frame: [FRAMES, 4, 4] float64"""
    start, increment = TRAJECTORIES[name]
    out = [cases.offset(*start).astype(np.float64)]
    D = cases.offset(*increment).astype(np.float64)
    for _ in range(1, FRAMES):
        out.append(out[-1] @ D)
    out = np.stack(out)
    out.setflags(write=False)
    return out


def true_poses(name):
    """the camera in the world at every frame, G * local: [FRAMES, 4, 4] float64"""
    return G @ local_poses(name)


@functools.lru_cache(maxsize=None)
def frames(name, depth_type):
    """the depth images of a trajectory, [FRAMES, ROWS, COLS]: float32 metres, or uint16 millimetres (scale 1e-3).  Shared by the
    tests: do not write into it"""
    out = np.stack([cases.render(P)[0] for P in local_poses(name)])
    if depth_type == "u16":
        out = cases.to_u16(out)
    for k in EMPTY[name]:
        out[k] = 0
    out.setflags(write=False)
    return out


def to_local(points_world):
    """[n, 3] world points in the scene's frame (float64)"""
    p = np.asarray(points_world, np.float64)
    return (p - G[:3, 3]) @ G[:3, :3]


def surface_distances(points_local):
    """for every point [n, 3] of the scene's frame the distance to each of the three planes and to the sphere, and each surface's unit
    normal towards the room: the planes' normals as they are written, the sphere's outward -> (distance [4, n], normal [4, n, 3])"""
    p = np.asarray(points_local, np.float64)
    distance, normal = [], []
    for n, point in cases.PLANES:
        n = np.asarray(n, np.float64) / np.linalg.norm(n)
        distance.append(np.abs((p - np.asarray(point, np.float64)) @ n))
        normal.append(np.broadcast_to(n, p.shape))
    r = p - np.asarray(cases.SPHERE[0], np.float64)
    length = np.linalg.norm(r, axis=1)
    distance.append(np.abs(length - cases.SPHERE[1]))
    with np.errstate(all="ignore"):
        normal.append(r / length[:, None])
    return np.stack(distance), np.stack(normal)


def scene_distance(points_local):
    """for every point [n, 3] of the scene's frame the distance to the nearest of the four surfaces and that surface's unit normal
    towards the room -> (distance [n], normal [n, 3])"""
    distance, normal = surface_distances(points_local)
    nearest = np.argmin(distance, axis=0)
    at = np.arange(distance.shape[1])
    return distance[nearest, at], normal[nearest, at]
