"""The scene clipper's rule (csrc/scene_clip.hip, SceneClipperProjective3D::compute) stated twice, in numpy, without a GPU.

clip()   restates the kernel in float32, one two-operand operation at a time and in the kernel's order (numpy rounds every float32
         operation on its own, there is no contraction), with the pose composed and inverted as csrc/prs_se3.h does it.  It is the
         expectation of the GPU tests: coordinates bit for bit, descriptors, indices, count and status.
inside() is the independent statement of the frustum: depth and pixel of a point in float64 for the identity pose, then the
         inequalities.  It shares no expression with clip().  It is meaningful where every float32 step of clip() is exact, which
         the planted points of tests/scene_clip_cases.py are by construction; elsewhere the two may differ by a rounding.

A projector is anything with fx, fy, cx, cy, canvas_cols, canvas_rows, range_min and range_max (oracle.Projector, _lib.Projector).
"""
import numpy as np

OK, WARN_EMPTY_INPUT, WARN_NO_PROJECTION = 0, 1, 32
F = np.float32
CANONICAL_NAN = np.uint32(0x7FC00000)


def se3_mul(A, B):
    """prs_se3.h se3_mul: C = A * B, rows 0..2, bottom row (0, 0, 0, 1)"""
    A, B = np.asarray(A, F).reshape(4, 4), np.asarray(B, F).reshape(4, 4)
    Cm = np.zeros((4, 4), F)
    for i in range(3):
        for j in range(3):
            Cm[i, j] = F(F(A[i, 0] * B[0, j]) + F(A[i, 1] * B[1, j])) + F(A[i, 2] * B[2, j])
        Cm[i, 3] = F(F(F(A[i, 0] * B[0, 3]) + F(A[i, 1] * B[1, 3])) + F(A[i, 2] * B[2, 3])) + A[i, 3]
    Cm[3, 3] = F(1)
    return Cm


def se3_inverse(T):
    """prs_se3.h se3_inverse: [R^T | -R^T t]"""
    T = np.asarray(T, F).reshape(4, 4)
    Ti = np.zeros((4, 4), F)
    tx, ty, tz = T[0, 3], T[1, 3], T[2, 3]
    for i in range(3):
        r0, r1, r2 = T[0, i], T[1, i], T[2, i]
        Ti[i, 0], Ti[i, 1], Ti[i, 2] = r0, r1, r2
        Ti[i, 3] = -F(F(F(r0 * tx) + F(r1 * ty)) + F(r2 * tz))
    Ti[3, 3] = F(1)
    return Ti


def sensor_differs(sensor_in_robot):
    """the reference's matrix operator!= (scene_clipper_projective_3d.cpp:61): element-wise, so -0.0 counts as 0"""
    S = np.asarray(sensor_in_robot, F).reshape(4, 4)
    return bool((S != np.eye(4, dtype=F)).any())


def _affine(M, x, y, z):
    return [F(F(F(M[r, 0] * x) + F(M[r, 1] * y)) + F(M[r, 2] * z)) + M[r, 3] for r in range(3)]


def rejections(projector, robot_in_local_map, sensor_in_robot, xyz):
    """the six value comparisons of the keep rule, each on its own, in float32: dict name -> bool [n] (True = this comparison
    rejects the row), plus the camera-frame coordinates.  A NaN makes every comparison false."""
    p = projector
    W = se3_inverse(se3_mul(robot_in_local_map, sensor_in_robot))
    pts = np.asarray(xyz, F).reshape(-1, np.shape(xyz)[-1])
    with np.errstate(all="ignore"):
        x, y, z = _affine(W, pts[:, 0], pts[:, 1], pts[:, 2])
        hx = F(F(p.fx) * x) + F(F(p.cx) * z)
        hy = F(F(p.fy) * y) + F(F(p.cy) * z)
        u = hx / z
        v = hy / z
        rej = {"z<min": z < F(p.range_min), "z>max": z > F(p.range_max), "u<0": u < F(0), "u>=cols": u >= F(p.canvas_cols),
               "v<0": v < F(0), "v>=rows": v >= F(p.canvas_rows)}
    return rej, (x, y, z)


def clip(projector, robot_in_local_map, sensor_in_robot, xyzw, desc=None, n_opt=None):
    """-> (clipped_xyzw [m,4] float32, clipped_desc [m,32] | None, global_indices [m] int32, m, status)"""
    xyzw = np.asarray(xyzw, F).reshape(-1, 4)
    n = xyzw.shape[0]
    if n == 0:  # :21-28: a warning, nothing is written
        return np.zeros((0, 4), F), (None if desc is None else np.zeros((0, 32), np.uint8)), np.zeros(0, np.int32), 0, WARN_EMPTY_INPUT
    rej, (x, y, z) = rejections(projector, robot_in_local_map, sensor_in_robot, xyzw)
    keep = np.ones(n, bool)
    for r in rej.values():
        keep &= ~r
    if sensor_differs(sensor_in_robot):  # kept points go on to the robot frame (:61-63)
        with np.errstate(all="ignore"):
            x, y, z = _affine(np.asarray(sensor_in_robot, F).reshape(4, 4), x, y, z)
    w = xyzw[:, 3]
    if n_opt is not None:  # aligner_slice_processor_projective.cpp:46-52 through the 4096-entry table
        from srrg2_proslam_amd import ops
        w = ops.info_scale_from_nopt(np.minimum(np.asarray(n_opt, np.uint32).reshape(n), np.uint32(4095)))
    idx = np.flatnonzero(keep).astype(np.int32)
    out = np.stack([x, y, z, w], axis=-1).astype(F)[idx]
    m = len(idx)
    return out, (None if desc is None else np.asarray(desc, np.uint8).reshape(n, 32)[idx].copy()), idx, m, (OK if m else WARN_NO_PROJECTION)


def inside(projector, xyz):
    """float64, identity pose: is the point in [range_min, range_max] and its pixel in [0, cols) x [0, rows)"""
    p = projector
    q = np.asarray(xyz, np.float64).reshape(-1, np.shape(xyz)[-1])
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        u = (float(p.fx) * x + float(p.cx) * z) / z
        v = (float(p.fy) * y + float(p.cy) * z) / z
    return ((z >= float(p.range_min)) & (z <= float(p.range_max)) & (u >= 0.0) & (u < float(p.canvas_cols))
            & (v >= 0.0) & (v < float(p.canvas_rows)))


def bits(a):
    """float32 values as uint32 patterns, every NaN as one pattern: IEEE 754 leaves sign and payload of a NaN that an operation
    produces to the implementation (0 * inf is 0xFFC00000 on x86 and 0x7FC00000 on the device), every other value is compared bit
    for bit, signed zeros included"""
    a = np.ascontiguousarray(a, F)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = CANONICAL_NAN
    return b
