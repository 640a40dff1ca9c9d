"""The TSDF raycast's rule (include/proslam_hip_tsdf_raycast.h, "TSDF raycast") restated in numpy: which views are skipped, a pixel's
ray, its stretch inside the box of the voxel centres, the samples and their validity, the hit, the depth, the normal, the counts and the
per-sequence refusal.  Explicit float32 operations in the order the header writes them, vectorised over the pixels and sequential over
the samples of a ray.  BUILD-DEFINED: the reference has no dense stage; this file is the specification the kernels are compared with,
byte for byte.  Test infrastructure only."""
import numpy as np

from depth_cloud_ref import frame_pose, se3_mul

PRS_OK, PRS_ERR_RANGE = 0, -4
F = np.float32
FLT_MAX = np.finfo(np.float32).max
MAX_STEPS = F(1048576.0)


def params(camera, voxel_size=0.02, step=0.02, min_weight=1.0, range_min=0.1, range_max=10.0, sensor_in_robot=None):
    S = np.eye(4, dtype=F) if sensor_in_robot is None else np.asarray(sensor_in_robot, F).reshape(4, 4)
    return dict(fx=F(camera["fx"]), fy=F(camera["fy"]), cx=F(camera["cx"]), cy=F(camera["cy"]), range_min=F(range_min),
                range_max=F(range_max), sensor_in_robot=S.copy(), voxel_size=F(voxel_size), step=F(step), min_weight=F(min_weight))


def refused(p, dims):
    """whether the call refuses these parameters for a volume of dims = (nx, ny, nz) voxels with PRS_ERR_RANGE"""
    values = [p[k] for k in ("fx", "fy", "cx", "cy", "range_min", "range_max", "voxel_size", "step", "min_weight")]
    if not (np.isfinite(values).all() and np.isfinite(p["sensor_in_robot"]).all()):
        return True
    if p["range_min"] < 0 or p["range_min"] > p["range_max"] or not p["voxel_size"] > 0 or not p["step"] > 0 or min(dims) < 1:
        return True
    with np.errstate(all="ignore"):
        steps = ((F(dims[0]) + F(dims[1])) + F(dims[2])) * p["voxel_size"] / p["step"]
    assert steps.dtype == F
    return not steps <= MAX_STEPS


def lerp(p, q, f):
    return p + f * (q - p)


def sample(volume, g, min_weight, slab=None):
    """the sample rule at the grid coordinates g = (g0, g1, g2), float32 arrays of one shape -> (valid, value).  slab: None, or
    (k0, nz): volume holds the layers from k0 on of a volume of nz layers whose other voxels are all-zero bytes"""
    vol = np.asarray(volume, F)
    k0, nz = (0, vol.shape[0]) if slab is None else slab
    dims = (vol.shape[2], vol.shape[1], nz)
    shape = g[0].shape
    if min(dims) < 2:
        return np.zeros(shape, bool), np.zeros(shape, F)
    with np.errstate(all="ignore"):
        i = [np.floor(x) for x in g]
        valid = np.ones(shape, bool)
        for a in range(3):
            valid &= np.isfinite(g[a]) & (i[a] >= F(0)) & (i[a] <= F(dims[a] - 2))
        j = [np.where(valid, x, F(0)).astype(np.int64) for x in i]
        for a in range(3):
            valid &= j[a] <= dims[a] - 2
        j = [np.where(valid, x, 0) for x in j]

        def corner(dx, dy, dz):
            k = j[2] + dz - k0
            held = (k >= 0) & (k < vol.shape[0])
            return np.where(held[..., None], vol[np.where(held, k, 0), j[1] + dy, j[0] + dx], F(0))
        c = {(dx, dy, dz): corner(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
        for cell in c.values():
            valid &= cell[..., 1] >= min_weight
        f = [g[a] - i[a] for a in range(3)]
        x = {(dy, dz): lerp(c[0, dy, dz][..., 0], c[1, dy, dz][..., 0], f[0]) for dz in (0, 1) for dy in (0, 1)}
        y = {dz: lerp(x[0, dz], x[1, dz], f[1]) for dz in (0, 1)}
        value = lerp(y[0], y[1], f[2])
    assert value.dtype == F
    return valid, np.where(valid, value, F(0))


def grid_of(T, dw, l, origin, vs):
    return [((T[a, 3] + l * dw[a]) - origin[a]) / vs - F(0.5) for a in range(3)]


def render(T, p, origin, volume, v, u, slab=None):
    """the pixels (v, u) (integer arrays of one shape) of the view with camera-to-world transform T [4, 4] float32
    -> (depth, normal [..., 4]) float32.  slab: as in sample()"""
    vol = np.asarray(volume, F)
    dims = (vol.shape[2], vol.shape[1], vol.shape[0] if slab is None else slab[1])
    o = np.asarray(origin, F)
    vs, step = p["voxel_size"], p["step"]
    v, u = np.asarray(v), np.asarray(u)
    shape = u.shape
    with np.errstate(all="ignore"):
        dc0 = (u.astype(F) - p["cx"]) / p["fx"]
        dc1 = (v.astype(F) - p["cy"]) / p["fy"]
        dw = [(T[a, 0] * dc0 + T[a, 1] * dc1) + T[a, 2] * F(1) for a in range(3)]
        l_in, l_out = np.full(shape, p["range_min"], F), np.full(shape, p["range_max"], F)
        miss = np.zeros(shape, bool)
        for a in range(3):
            lo = o[a] + F(0.5) * vs
            hi = o[a] + (F(dims[a]) - F(0.5)) * vs
            flat = dw[a] == 0
            miss |= flat & ((T[a, 3] < lo) | (T[a, 3] > hi))
            t1, t2 = (lo - T[a, 3]) / dw[a], (hi - T[a, 3]) / dw[a]
            near, far = np.where(t2 < t1, t2, t1), np.where(t2 < t1, t1, t2)
            l_in = np.where(~flat & (near > l_in), near, l_in)
            l_out = np.where(~flat & (far < l_out), far, l_out)
        q = (l_out - l_in) / step
        assert q.dtype == F
        marched = ~miss & (l_in <= l_out) & (q >= 0)
        trips = np.where(marched, np.where(q < MAX_STEPS, q, MAX_STEPS).astype(np.int64) + 2, 0)
        live = trips > 0
        hit = np.zeros(shape, bool)
        prev_valid, prev_t, prev_l, l_star = np.zeros(shape, bool), np.zeros(shape, F), np.zeros(shape, F), np.zeros(shape, F)
        k = 0
        while live.any():
            l = l_in + F(k) * step
            live = live & (l <= l_out)
            valid, t = sample(vol, grid_of(T, dw, l, o, vs), p["min_weight"], slab)
            end = live & valid & (t <= 0)
            now = end & prev_valid & (prev_t > 0)
            l_star = np.where(now, prev_l + step * (prev_t / (prev_t - t)), l_star)
            hit |= now
            go = live & ~end
            prev_valid, prev_t, prev_l = np.where(go, valid, prev_valid), np.where(go, t, prev_t), np.where(go, l, prev_l)
            live = go & (k + 1 < trips)
            k += 1
        assert l_star.dtype == F
        depth = np.where(hit & (l_star >= p["range_min"]) & (l_star <= p["range_max"]), l_star, F(0))
        counted = depth > 0
        g = grid_of(T, dw, depth, o, vs)
        m, ok = [], counted.copy()
        for a in range(3):
            up, down = list(g), list(g)
            up[a], down[a] = g[a] + F(1), g[a] - F(1)
            (v_hi, hi), (v_lo, lo) = sample(vol, up, p["min_weight"], slab), sample(vol, down, p["min_weight"], slab)
            ok &= v_hi & v_lo
            m.append(hi - lo)
        len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
        ok &= (len2 > 0) & (len2 <= FLT_MAX)
        length = np.sqrt(len2)
        qn = [x / length for x in m]
        normal = np.zeros(shape + (4,), F)
        for i in range(3):
            normal[..., i] = np.where(ok, (T[0, i] * qn[0] + T[1, i] * qn[1]) + T[2, i] * qn[2], F(0))
        normal[..., 3] = np.where(ok, F(1), F(0))
        assert len2.dtype == F and length.dtype == F and depth.dtype == F
    return depth.astype(F), normal


def view_transform(seq, r, p):
    """T of view r of a sequence -- pose [pose_stride, 16] and optionally view_index [views] --, or None when the view is skipped"""
    _, pose = frame_pose(dict(pose=seq["pose"], frame_index=seq.get("view_index")), r)
    return None if pose is None else se3_mul(pose, p["sensor_in_robot"])


def raycast(seq, p, origin, volume, views, rows, cols, before=None, pixels=None, slab=None):
    """seq: one sequence -- pose [pose_stride, 16] float32, optionally view_index [views] and n_views (absent or None: views).
    p: params().  volume: [nz, ny, nx, 2] float32.  before: dict of depth [views, rows, cols], normal [views, rows, cols, 4] and n_hit
    [views] as they stand (None: zeros).  pixels: None, or (v, u) integer arrays: only these pixels are rendered, the outputs are
    depth [views, len], normal [views, len, 4] and n_hit counts them alone.  slab: as in sample().
    -> dict(status, n_skipped, depth, normal, n_hit): the arrays after the call"""
    before = before or {}
    if pixels is None:
        v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    else:
        v, u = (np.asarray(x) for x in pixels)
    shape = v.shape
    out = dict(depth=np.array(before.get("depth", np.zeros((views,) + shape, F)), F, copy=True),
               normal=np.array(before.get("normal", np.zeros((views,) + shape + (4,), F)), F, copy=True),
               n_hit=np.array(before.get("n_hit", np.zeros(views, np.int32)), np.int32, copy=True), n_skipped=0)
    n = views if seq.get("n_views") is None else int(seq["n_views"])
    if n < 0 or n > views:
        out["status"] = PRS_ERR_RANGE
        return out
    out["status"] = PRS_OK
    for r in range(n):
        T = view_transform(seq, r, p)
        if T is None:
            out["n_skipped"] += 1
            out["depth"][r], out["normal"][r], out["n_hit"][r] = F(0), F(0), 0
            continue
        out["depth"][r], out["normal"][r] = render(T, p, origin, volume, v, u, slab)
        out["n_hit"][r] = int((out["depth"][r] > 0).sum())
    return out
