"""The world voxel filter's rule (include/proslam_hip.h, "World voxel filter") restated in numpy for one sequence: which rows are
dropped, the voxel of a row, the representative, the position in both modes, the order, truncation, the count-only call and the table
overflow.  BUILD-DEFINED: the reference writes no map; this file is what the kernels are compared with, byte for byte.  Test
infrastructure only."""
import numpy as np

PRS_OK, PRS_ERR_CAPACITY, PRS_ERR_RANGE = 0, -2, -4
REPRESENTATIVE, MEAN = 0, 1
HALF = 1 << 20
FRACTION = 1073741824.0


def params(voxel_size, position=REPRESENTATIVE):
    return dict(voxel_size=np.float32(voxel_size), position=int(position))


def voxel_index(x, s):
    """float32 coordinates (any shape) and the float64 voxel size -> k = floor((double) x / s) as float64"""
    with np.errstate(all="ignore"):
        return np.floor(np.asarray(x, np.float32).astype(np.float64) / np.float64(s))


def voxel_key(k):
    """int64 k [n, 3] inside the grid -> uint64 keys"""
    u = (np.asarray(k, np.int64) + HALF).astype(np.uint64)
    return (u[:, 0] << np.uint64(42)) | (u[:, 1] << np.uint64(21)) | u[:, 2]


def rank_key(n_opt, i):
    """the packed rank whose minimum over a voxel's rows names the representative"""
    return ((~np.asarray(n_opt, np.uint32)).astype(np.uint64) << np.uint64(32)) | np.asarray(i, np.uint64)


def world_voxel(cloud, p, out_stride, table_stride=None):
    """cloud: one sequence as numpy arrays -- in_stride, n (in_n[b]), xyz [in_stride, 4] float32 and optionally n_opt [in_stride]
    uint32, desc [in_stride, 32], node, row [in_stride] (absent or None: the input is not set).  p: params().  out_stride: rows of the
    output, or None for the count-only call.  table_stride: the slots of the table, None = never too few.
    -> dict(status, n_out, n_voxels, n_nonfinite, n_outside, xyz [n_out, 4], index, count, and desc, node, row, n_opt where the input
            is set)"""
    N, n = int(cloud["in_stride"]), int(cloud["n"])
    have = [k for k in ("desc", "node", "row", "n_opt") if cloud.get(k) is not None]
    out = dict(status=PRS_ERR_RANGE, n_out=0, n_voxels=0, n_nonfinite=0, n_outside=0, xyz=np.zeros((0, 4), np.float32),
               index=np.zeros(0, np.int32), count=np.zeros(0, np.int32))
    for k in have:
        out[k] = np.asarray(cloud[k])[:0]
    if n < 0 or n > N:
        return out
    s = np.float64(np.float32(p["voxel_size"]))
    x = np.asarray(cloud["xyz"], np.float32)[:n]
    n_opt = np.asarray(cloud["n_opt"])[:n].astype(np.uint32) if cloud.get("n_opt") is not None else np.zeros(n, np.uint32)
    finite = np.isfinite(x[:, :3]).all(axis=1)
    k = voxel_index(x[:, :3], s)
    with np.errstate(invalid="ignore"):
        inside = finite & ((k >= -HALF) & (k < HALF)).all(axis=1)
    out.update(n_nonfinite=int((~finite).sum()), n_outside=int((finite & ~inside).sum()))
    rows = np.nonzero(inside)[0]
    ki = k[rows].astype(np.int64)
    keys = voxel_key(ki)
    uniq, inv, counts = np.unique(keys, return_inverse=True, return_counts=True)
    if table_stride is not None and uniq.size > int(table_stride):
        out.update(status=PRS_ERR_CAPACITY, n_voxels=-1)
        return out
    # the representative: the minimum of the packed rank per voxel
    rank = rank_key(n_opt[rows], rows)
    best = np.full(uniq.size, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(best, inv, rank)
    rep = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)  # input row of every voxel's representative
    order = np.argsort(rep, kind="stable")                   # voxels by their representative's row
    rep, counts_o = rep[order], counts[order].astype(np.int32)
    xyz = x[rep].copy()
    if p["position"] == MEAN:
        with np.errstate(all="ignore"):
            f = x[rows, :3].astype(np.float64) - ki.astype(np.float64) * s
            q = np.rint((f / s) * FRACTION).astype(np.int64)
        S = np.zeros((uniq.size, 3), np.int64)
        np.add.at(S, inv, q)
        S = S[order]
        k_rep = voxel_index(x[rep, :3], s)
        m = (k_rep + (S.astype(np.float64) / counts_o.astype(np.float64)[:, None]) / FRACTION) * s
        xyz[:, :3] = m.astype(np.float32)
    total = int(uniq.size)
    out.update(n_voxels=total, status=PRS_OK)
    if out_stride is None:
        return out
    j = min(total, int(out_stride))
    out.update(n_out=j, xyz=xyz[:j], index=rep[:j].astype(np.int32), count=counts_o[:j],
               status=PRS_ERR_CAPACITY if total > int(out_stride) else PRS_OK)
    for name in have:
        out[name] = np.asarray(cloud[name])[rep[:j]]
    return out


def host_route(xyz, n_opt, voxel_size):
    """the route the device call replaces, for tools/bench_world_voxel.py: a host cloud (WorldMapBatch.cloud_of) through a sort by
    voxel key -> the rows of the representatives, ascending (the REPRESENTATIVE position)"""
    c = dict(in_stride=xyz.shape[0], n=xyz.shape[0], xyz=xyz, n_opt=n_opt)
    return world_voxel(c, params(voxel_size), xyz.shape[0])["index"]
