"""The TSDF fusion's rule (include/proslam_hip_tsdf.h, "TSDF fusion") restated in numpy: which frames are skipped, which voxels an
image updates and how, the counts and the per-sequence refusal of the integrate call; the crossings, their points, normals and cells,
their order, truncation at out_stride and the count-only call of the surface call.  Explicit float32 operations in the order the
header writes them, vectorised over the voxels and sequential over the frames.  BUILD-DEFINED: the reference has no dense stage; this
file is the specification the kernels are compared with, byte for byte.  Test infrastructure only."""
import numpy as np

from depth_cloud_ref import frame_pose, se3_mul

PRS_OK, PRS_ERR_CAPACITY, PRS_ERR_RANGE = 0, -2, -4
F = np.float32
FLT_MAX = np.finfo(np.float32).max


def params(camera, voxel_size=0.02, truncation=0.08, max_weight=64.0, min_weight=1.0, range_min=0.1, range_max=10.0, scale=1.0,
           sensor_in_robot=None):
    S = np.eye(4, dtype=F) if sensor_in_robot is None else np.asarray(sensor_in_robot, F).reshape(4, 4)
    return dict(fx=F(camera["fx"]), fy=F(camera["fy"]), cx=F(camera["cx"]), cy=F(camera["cy"]), range_min=F(range_min),
                range_max=F(range_max), scale=F(scale), sensor_in_robot=S.copy(), voxel_size=F(voxel_size), truncation=F(truncation),
                max_weight=F(max_weight), min_weight=F(min_weight))


def se3_inverse(T):
    """prs_se3.h se3_inverse on a float32 [4, 4]: [R^T | -((r0 tx + r1 ty) + r2 tz)]"""
    T = np.asarray(T, F).reshape(4, 4)
    Ti = np.zeros((4, 4), F)
    Ti[3, 3] = F(1)
    tx, ty, tz = T[0, 3], T[1, 3], T[2, 3]
    with np.errstate(all="ignore"):
        for i in range(3):
            r0, r1, r2 = T[0, i], T[1, i], T[2, i]
            Ti[i, 0], Ti[i, 1], Ti[i, 2] = r0, r1, r2
            Ti[i, 3] = -F(F(F(r0 * tx) + F(r1 * ty)) + F(r2 * tz))
    return Ti


def centres(shape, origin, voxel_size, k0=0):
    """(c0 [1, 1, nx], c1 [1, ny, 1], c2 [nk, 1, 1]) of the voxels (i, j, k0 + k): o + ((float) index + 0.5f) * voxel_size"""
    nk, ny, nx = shape
    o = np.asarray(origin, F)
    half = F(0.5)
    c0 = o[0] + (np.arange(nx).astype(F) + half) * voxel_size
    c1 = o[1] + (np.arange(ny).astype(F) + half) * voxel_size
    c2 = o[2] + (np.arange(k0, k0 + nk).astype(F) + half) * voxel_size
    assert c0.dtype == F and c1.dtype == F and c2.dtype == F
    return c0[None, None, :], c1[None, :, None], c2[:, None, None]


def integrate_image(tsdf, w, image, Ti, p, c):
    """one image into (tsdf, w) [nk, ny, nx] in place -> the voxels it updated"""
    rows, cols = image.shape
    one = F(1)
    with np.errstate(all="ignore"):
        q = [((Ti[i, 0] * c[0] + Ti[i, 1] * c[1]) + Ti[i, 2] * c[2]) + Ti[i, 3] for i in range(3)]
        z = np.broadcast_to(q[2], tsdf.shape)
        m = (z > 0) & (z >= p["range_min"]) & (z <= p["range_max"])
        uf = np.floor((q[0] / z * p["fx"] + p["cx"]) + F(0.5))
        vf = np.floor((q[1] / z * p["fy"] + p["cy"]) + F(0.5))
        assert uf.dtype == F and vf.dtype == F
        m = m & (uf >= 0) & (uf < F(cols)) & (vf >= 0) & (vf < F(rows))
        u, v = np.where(m, uf, F(0)).astype(np.int64), np.where(m, vf, F(0)).astype(np.int64)
        raw = np.asarray(image)[v, u].astype(F)  # a 16-bit value converts exactly
        d = p["scale"] * raw
        m = m & (raw > 0) & (d >= p["range_min"]) & (d <= p["range_max"])
        sdf = d - z
        m = m & (sdf >= -p["truncation"])
        t = sdf / p["truncation"]
        t = np.where(t > one, one, t)
        w1 = w + one
        new = (tsdf * w + t) / w1
        assert new.dtype == F and w1.dtype == F
        tsdf[...] = np.where(m, new, tsdf)
        w[...] = np.where(m, np.where(w1 > p["max_weight"], p["max_weight"], w1), w)
    return int(m.sum())


def integrate(seq, p, origin, volume, n_updates=None, slab=None):
    """seq: one sequence -- depth [frames, rows, cols] (uint16 or float32), n_images (absent or None: frames), pose [pose_stride, 16]
    float32 and optionally frame_index [frames].  p: params().  origin: three floats or more.  volume: [nz, ny, nx, 2] float32 as it
    stands before the call.  n_updates: [frames] as it stands (None: zeros).  slab: None, or (k0, k1): volume holds the layers
    k0 .. k1 - 1 of a taller volume, and n_updates counts these layers alone.
    -> dict(status, volume, n_updates, n_skipped): the arrays after the call"""
    depth = np.asarray(seq["depth"])
    frames = depth.shape[0]
    n_img = frames if seq.get("n_images") is None else int(seq["n_images"])
    out = dict(volume=np.array(volume, F, copy=True),
               n_updates=np.zeros(frames, np.int32) if n_updates is None else np.array(n_updates, np.int32, copy=True), n_skipped=0)
    if n_img < 0 or n_img > frames:
        out["status"] = PRS_ERR_RANGE
        return out
    out["status"] = PRS_OK
    out["n_updates"][:] = 0
    tsdf, w = out["volume"][..., 0].copy(), out["volume"][..., 1].copy()
    c = centres(tsdf.shape, origin, p["voxel_size"], 0 if slab is None else slab[0])
    for f in range(n_img):
        _, pose = frame_pose(seq, f)
        if pose is None:
            out["n_skipped"] += 1
            continue
        Ti = se3_inverse(se3_mul(pose, p["sensor_in_robot"]))
        out["n_updates"][f] = integrate_image(tsdf, w, depth[f], Ti, p, c)
    out["volume"][..., 0], out["volume"][..., 1] = tsdf, w
    return out


def surface(volume, p, origin, out_stride, before=None, count_only=False):
    """volume [nz, ny, nx, 2] float32; before: dict of xyz, normal [out_stride, 4] and cell [out_stride] as they stand (None: zeros).
    -> dict(status, n_out, n_total, xyz, normal, cell): the whole output arrays after the call"""
    vol = np.asarray(volume, F)
    nz, ny, nx = vol.shape[:3]
    cap = max(int(out_stride), 0)
    before = before or {}
    out = dict(xyz=np.array(before.get("xyz", np.zeros((cap, 4), F)), F, copy=True),
               normal=np.array(before.get("normal", np.zeros((cap, 4), F)), F, copy=True),
               cell=np.array(before.get("cell", np.zeros(cap, np.int32)), np.int32, copy=True))
    t, w = vol[..., 0], vol[..., 1]
    vs = p["voxel_size"]
    with np.errstate(all="ignore"):
        observed = w >= p["min_weight"]
        band = observed & (np.abs(t) < F(1))
        neg = t < F(0)
        cross = np.zeros((nz, ny, nx, 3), bool)  # [k][j][i][e]: raster order, then the axes
        cross[:, :, :-1, 0] = band[:, :, :-1] & band[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
        cross[:, :-1, :, 1] = band[:, :-1, :] & band[:, 1:, :] & (neg[:, :-1, :] != neg[:, 1:, :])
        cross[:-1, :, :, 2] = band[:-1, :, :] & band[1:, :, :] & (neg[:-1, :, :] != neg[1:, :, :])
        k, j, i, e = np.nonzero(cross)
        total = int(k.size)
        out["n_total"] = total
        if count_only:
            out.update(status=PRS_OK, n_out=0)
            return out
        n_out = min(total, cap)
        out.update(status=PRS_ERR_CAPACITY if total > cap else PRS_OK, n_out=n_out)
        k, j, i, e = k[:n_out], j[:n_out], i[:n_out], e[:n_out]
        a = np.stack([i, j, k], axis=1)  # [n, 3] in the order of the axes
        step = np.eye(3, dtype=np.int64)[e]
        n = a + step
        at = lambda arr, q: arr[q[:, 2], q[:, 1], q[:, 0]]  # noqa: E731
        ta, tn, wa, wn = at(t, a), at(t, n), at(w, a), at(w, n)
        s = ta / (ta - tn)
        o = np.asarray(origin, F)[:3]
        c = o[None, :] + (a.astype(F) + F(0.5)) * vs
        assert c.dtype == F and s.dtype == F
        moved = c + (s * vs)[:, None]
        xyz = np.where(step.astype(bool), moved, c)
        out["xyz"][:n_out, :3] = xyz
        out["xyz"][:n_out, 3] = np.where(wn < wa, wn, wa)
        at_n = np.abs(tn) < np.abs(ta)
        g = np.where(at_n[:, None], n, a)
        tg = np.where(at_n, tn, ta)
        dims = np.array([nx, ny, nz])
        m = np.zeros((n_out, 3), F)
        for d in range(3):
            unit = np.eye(3, dtype=np.int64)[d]
            up, down = g + unit, g - unit
            has_up, has_down = up[:, d] < dims[d], down[:, d] >= 0
            up, down = np.where(has_up[:, None], up, g), np.where(has_down[:, None], down, g)
            hi = np.where(has_up & at(observed, up), at(t, up), tg)
            lo = np.where(has_down & at(observed, down), at(t, down), tg)
            m[:, d] = hi - lo
        len2 = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
        ok = (len2 > 0) & (len2 <= FLT_MAX)
        length = np.sqrt(len2)
        assert len2.dtype == F and length.dtype == F
        out["normal"][:n_out, :3] = np.where(ok[:, None], m / length[:, None], F(0))
        out["normal"][:n_out, 3] = np.where(ok, F(1), F(0))
        out["cell"][:n_out] = (3 * ((k * ny + j) * nx + i) + e).astype(np.int32)
    return out
