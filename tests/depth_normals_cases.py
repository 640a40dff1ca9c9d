"""Depth images for the depth normals' tests (tests/test_depth_normals_ref.py on the CPU, tests/test_depth_normals_gpu.py on the
device): analytic surfaces rendered in float64 and rounded once to the depth type, and images of the values the validity test must
drop.  Test infrastructure only."""
import numpy as np

F = np.float32
K = dict(fx=525.0, fy=-519.5, cx=18.3, cy=14.7)      # the dense cloud tests' camera: a negative fy, a principal point off the centre
K_WIDE = dict(fx=60.0, fy=60.0, cx=31.5, cy=23.5)   # a short focal length: a sphere fills a 64 x 48 image


def rays(rows, cols, camera):
    """((u - cx) / fx, (v - cy) / fy) of every pixel in float64, each [rows, cols]"""
    kx = (np.arange(cols, dtype=np.float64) - np.float64(F(camera["cx"]))) / np.float64(F(camera["fx"]))
    ky = (np.arange(rows, dtype=np.float64) - np.float64(F(camera["cy"]))) / np.float64(F(camera["fy"]))
    return np.broadcast_to(kx[None, :], (rows, cols)), np.broadcast_to(ky[:, None], (rows, cols))


def plane_depth(rows, cols, camera, normal, offset):
    """float32 depths [rows, cols] of the plane normal . X = offset -> (depth, the unit normal that faces the camera)"""
    kx, ky = rays(rows, cols, camera)
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    d = offset / (n[0] * kx + n[1] * ky + n[2])
    assert (d > 0).all()
    return d.astype(F), (-n if n[2] > 0 else n)


def sphere_depth(rows, cols, camera, centre_z, radius):
    """float32 depths [rows, cols] of the sphere of this radius around (0, 0, centre_z), 0 where a ray misses it or grazes it
    -> (depth, the outward unit normals [rows, cols, 3], the mask of the pixels whose rays hit the sphere well inside its rim)"""
    kx, ky = rays(rows, cols, camera)
    g2 = kx * kx + ky * ky + 1.0
    disc = centre_z * centre_z - g2 * (centre_z * centre_z - radius * radius)
    hit = disc > 0.25 * radius * radius  # away from the silhouette, where the depth changes fast from pixel to pixel
    d = np.where(hit, (centre_z - np.sqrt(np.maximum(disc, 0.0))) / g2, 0.0)
    X = np.stack([kx * d, ky * d, d - centre_z], axis=-1) / radius
    return d.astype(F), X, hit


def step_image(rows, cols, near, far, at, vertical=True, dtype=F):
    """two fronto-parallel planes: depth `near` in the columns (vertical) or rows below `at`, `far` from `at` on"""
    d = np.full((rows, cols), near, dtype)
    if vertical:
        d[:, at:] = far
    else:
        d[at:, :] = far
    return d


ODD_F32 = [0.0, -0.0, np.nan, -1.0, np.inf, -np.inf, 1e-40, 3e38, 0.05, 10.5]  # none is a valid depth in metres within [0.1, 10]


def odd_values_image(rng, rows=12, cols=20):
    """a fronto-parallel plane at 2 m with a third of its pixels replaced by values the validity test drops -> (float32 image, the
    mask of the replaced pixels)"""
    d = np.full((rows, cols), 2.0, F)
    odd = rng.random((rows, cols)) < 1.0 / 3.0
    d[odd] = np.resize(np.array(ODD_F32, F), int(odd.sum()))
    return d, odd


def as_u16(depth_m):
    """metres to 16-bit millimetres, rounded to nearest (0 stays 0)"""
    return np.rint(np.asarray(depth_m, np.float64) * 1000.0).astype(np.uint16)


def random_depth(rng, shape, depth_type, invalid=0.1):
    """a rough surface between 1 and 3 m with smooth patches, steps and a tenth of invalid pixels: every branch of the rule occurs"""
    rows, cols = shape[-2:]
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    base = 2.0 + 0.01 * u + 0.02 * v + 0.5 * ((u // 7 + v // 5) % 2)  # tilted, with steps every few pixels
    d = base + rng.normal(0.0, 0.01, shape)
    d = np.where(rng.random(shape) < invalid, 0.0, d)
    return as_u16(d) if depth_type == "u16" else d.astype(F)
