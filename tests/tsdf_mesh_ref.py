"""The TSDF mesh's rule (include/proslam_hip_tsdf_mesh.h, "TSDF mesh") restated in numpy: surface nets over the crossings of
tests/tsdf_ref.py's surface call -- the active cubes and their order, a vertex as the mean of its cube's crossings and its normal as
their normalised sum, a quad around every interior crossing and its winding, truncation at the two strides, the status and the
count-only call.  The crossings, their points, normals and ids are tsdf_ref.surface's and nothing else; the sums run sequentially in
ascending id in explicit float32.  BUILD-DEFINED: the reference has no dense stage; this file is the specification the kernels are
compared with, byte for byte.  Test infrastructure only."""
import numpy as np

import tsdf_ref
from tsdf_ref import PRS_ERR_CAPACITY, PRS_OK, F, FLT_MAX


def crossings(volume, p, origin):
    """every taken crossing of the volume in ascending id -> (cell [n], xyz [n, 4], normal [n, 4]) as the surface call writes them"""
    vol = np.asarray(volume, F)
    voxels = vol.shape[0] * vol.shape[1] * vol.shape[2]
    s = tsdf_ref.surface(vol, p, origin, 3 * voxels)
    n = s["n_total"]
    assert s["status"] == PRS_OK and s["n_out"] == n
    return s["cell"][:n].astype(np.int64), s["xyz"][:n], s["normal"][:n]


def cubes_of(a, e, dims):
    """the cubes (as coordinate triples) that have the edge (a, e) among their twelve, in no particular order"""
    b, c = (e + 1) % 3, (e + 2) % 3
    out = []
    for db in (1, 0):
        for dc in (1, 0):
            q = list(a)
            q[b] -= db
            q[c] -= dc
            if all(0 <= q[d] < dims[d] - 1 for d in range(3)):
                out.append(tuple(q))
    return out


def mesh(volume, p, origin, vertex_stride, quad_stride, before=None, count_only=False):
    """volume [nz, ny, nx, 2] float32; before: dict of vertex, normal [vertex_stride, 4], quad [quad_stride, 4], cube [vertex_stride]
    and edge [quad_stride] as they stand (None: zeros).
    -> dict(status, n_vertices, n_vertices_total, n_quads, n_quads_total, vertex, normal, quad, cube, edge): the whole output arrays
    after the call"""
    vol = np.asarray(volume, F)
    nz, ny, nx = vol.shape[:3]
    dims = (nx, ny, nz)
    vcap, qcap = max(int(vertex_stride), 0), max(int(quad_stride), 0)
    before = before or {}
    out = dict(vertex=np.array(before.get("vertex", np.zeros((vcap, 4), F)), F, copy=True),
               normal=np.array(before.get("normal", np.zeros((vcap, 4), F)), F, copy=True),
               quad=np.array(before.get("quad", np.zeros((qcap, 4), np.int32)), np.int32, copy=True),
               cube=np.array(before.get("cube", np.zeros(vcap, np.int32)), np.int32, copy=True),
               edge=np.array(before.get("edge", np.zeros(qcap, np.int32)), np.int32, copy=True))
    cell, P, N = crossings(vol, p, origin)
    lin_of = lambda q: (q[2] * ny + q[1]) * nx + q[0]  # noqa: E731
    members = {}   # lin(q) of an active cube -> the rows of its taken crossings, ascending
    interior = []  # (row of the crossing, a, e) of the interior ones, ascending
    for row, cid in enumerate(cell.tolist()):
        lin, e = divmod(cid, 3)
        a = (lin % nx, (lin // nx) % ny, lin // (nx * ny))
        around = cubes_of(a, e, dims)
        for q in around:
            members.setdefault(lin_of(q), []).append(row)
        b, c = (e + 1) % 3, (e + 2) % 3
        if 1 <= a[b] <= dims[b] - 2 and 1 <= a[c] <= dims[c] - 2:
            assert len(around) == 4
            interior.append((row, a, e))
    active = sorted(members)  # ascending lin is the raster order: k outer, then j, then i
    rank = {lin: r for r, lin in enumerate(active)}
    out.update(n_vertices_total=len(active), n_quads_total=len(interior))
    if count_only:
        out.update(status=PRS_OK, n_vertices=0, n_quads=0)
        return out
    n_v, n_q = min(len(active), vcap), min(len(interior), qcap)
    out.update(status=PRS_ERR_CAPACITY if len(active) > vcap or len(interior) > qcap else PRS_OK, n_vertices=n_v, n_quads=n_q)
    with np.errstate(all="ignore"):
        for r, lin in enumerate(active[:n_v]):
            rows = members[lin]
            assert rows == sorted(rows) and 1 <= len(rows) <= 12
            m = F(len(rows))
            s, g = np.zeros(3, F), np.zeros(3, F)
            for row in rows:
                for d in range(3):
                    s[d] = s[d] + P[row, d]
                if N[row, 3] != 0:
                    for d in range(3):
                        g[d] = g[d] + N[row, d]
            out["vertex"][r] = (s[0] / m, s[1] / m, s[2] / m, m)
            len2 = F(F(g[0] * g[0]) + F(g[1] * g[1])) + F(g[2] * g[2])
            if len2 > 0 and len2 <= FLT_MAX:
                length = np.sqrt(len2)
                assert length.dtype == F
                out["normal"][r] = (g[0] / length, g[1] / length, g[2] / length, F(1))
            else:
                out["normal"][r] = 0
            out["cube"][r] = lin
    t = vol[..., 0]
    for r, (row, a, e) in enumerate(interior[:n_q]):
        b, c = (e + 1) % 3, (e + 2) % 3
        ub, uc = np.eye(3, dtype=np.int64)[b], np.eye(3, dtype=np.int64)[c]
        a = np.array(a, np.int64)
        q00, q10, q11, q01 = (rank[lin_of(q)] for q in (a - ub - uc, a - uc, a, a - ub))
        with np.errstate(all="ignore"):
            negative = bool(t[a[2], a[1], a[0]] < F(0))
        out["quad"][r] = (q00, q10, q11, q01) if negative else (q00, q01, q11, q10)
        out["edge"][r] = cell[row]
    return out


def triangles(quad):
    """[2 n, 3]: the triangles (v0, v1, v2) and (v0, v2, v3) of quad i at rows 2 i and 2 i + 1"""
    quad = np.asarray(quad)
    return quad[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3)


def edge_use(quad):
    """(undirected, directed): dictionaries from a mesh edge (a pair of vertex rows) to the number of quads that have it"""
    undirected, directed = {}, {}
    for v in np.asarray(quad).tolist():
        for a, b in zip(v, v[1:] + v[:1]):
            directed[(a, b)] = directed.get((a, b), 0) + 1
            key = (min(a, b), max(a, b))
            undirected[key] = undirected.get(key, 0) + 1
    return undirected, directed
