"""The world map's rule (include/proslam_hip.h, "World map") restated in numpy for one sequence: which maps are chosen, which rows
kept, the float64 world coordinates in the written operation order, the node-then-row order, truncation, the count-only call,
the bounds and refresh_state.  BUILD-DEFINED: the reference writes no map; this file is what the kernels are compared with, byte for
byte.  Test infrastructure only."""
import numpy as np

PRS_OK, PRS_ERR_CAPACITY, PRS_ERR_RANGE = 0, -2, -4


def params(min_n_opt=0, require_inlier=False, include_live=True, refresh_state=False):
    return dict(min_n_opt=int(min_n_opt), require_inlier=bool(require_inlier), include_live=bool(include_live),
                refresh_state=bool(refresh_state))


def world_rows(X16, coords):
    """float64 node pose [16] and float32 coords [n, 4] -> float32 [n, 3]: explicit two-operand float64 operations in the header's
    order, one rounding to float"""
    X = np.asarray(X16, np.float64).reshape(16)
    c = np.asarray(coords, np.float32)
    x, y, z = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64), c[:, 2].astype(np.float64)
    with np.errstate(all="ignore"):
        w = [(((X[4 * i + 0] * x + X[4 * i + 1] * y) + X[4 * i + 2] * z) + X[4 * i + 3]).astype(np.float32) for i in range(3)]
    return np.stack(w, axis=1)


def empty_bounds():
    return np.array([np.inf] * 3 + [-np.inf] * 3, np.float32)


def world_map(seq, p, out_stride):
    """seq: one sequence as numpy arrays --
         capacity, slot_stride, node_stride, n_nodes, cur_node, graph_X [node_stride, 16] float64, slot_of_node [node_stride],
         live = dict(coords [cap, 4], desc [cap, 32], n_opt [cap], inlier [cap], state [cap, 4], n_points),
         slots = dict(coords [S, cap, 4], desc [S, cap, 32], n_opt [S, cap], inlier [S, cap], state [S, cap, 4], n_points [S]).
    p: params().  out_stride: rows of the output, or None for the count-only call.
    -> dict(status, n_out, n_total, n_nonfinite, xyz [n_out, 4], desc, node, row, n_opt, bounds [6] or None (not written),
            live_state [cap, 4], slot_state [S, cap, 4] as the call leaves them)"""
    cap, S, NS = int(seq["capacity"]), int(seq["slot_stride"]), int(seq["node_stride"])
    live, slots = seq["live"], seq["slots"]
    out = dict(status=PRS_ERR_RANGE, n_out=0, n_total=0, n_nonfinite=0, xyz=np.zeros((0, 4), np.float32),
               desc=np.zeros((0, 32), np.uint8), node=np.zeros(0, np.int32), row=np.zeros(0, np.int32), n_opt=np.zeros(0, np.uint32),
               bounds=None, live_state=np.array(live["state"], np.float32, copy=True),
               slot_state=np.array(slots["state"], np.float32, copy=True))
    nn, cur = int(seq["n_nodes"]), int(seq["cur_node"])
    if nn < 1 or nn > NS or cur < 0 or cur >= nn:
        return out
    if p["include_live"] and not 0 <= int(live["n_points"]) <= cap:
        return out
    # the maps in node order: (node, source arrays, slot or None for the live map, n_points)
    chosen, claimed = [], set()
    for n in range(nn):
        if p["include_live"] and n == cur:
            chosen.append((n, live, None, int(live["n_points"])))
            continue
        s = int(seq["slot_of_node"][n])
        if s < 0:
            continue
        if s >= S or not 0 <= int(slots["n_points"][s]) <= cap or s in claimed:
            return out
        claimed.add(s)
        chosen.append((n, {k: slots[k][s] for k in ("coords", "desc", "n_opt", "inlier")}, s, int(slots["n_points"][s])))
    xyz, desc, node, row, n_opt = [], [], [], [], []
    n_nonfinite = 0
    for n, src, s, np_ in chosen:
        c = np.asarray(src["coords"], np.float32)[:np_]
        w = world_rows(seq["graph_X"][n], c)
        finite = np.isfinite(w).all(axis=1)
        nopt = np.asarray(src["n_opt"])[:np_].astype(np.uint32)
        passes = nopt >= np.uint32(p["min_n_opt"])
        if p["require_inlier"]:
            passes &= np.asarray(src["inlier"])[:np_] != 0
        n_nonfinite += int((passes & ~finite).sum())
        keep = np.nonzero(passes & finite)[0]
        row4 = np.concatenate([w[keep], c[keep, 3:4]], axis=1)  # the fourth column's bits are copied
        xyz.append(row4)
        desc.append(np.asarray(src["desc"], np.uint8)[:np_][keep])
        node.append(np.full(keep.size, n, np.int32))
        row.append(keep.astype(np.int32))
        n_opt.append(nopt[keep])
        if p["refresh_state"]:
            state = out["live_state"] if s is None else out["slot_state"][s]
            rows = np.nonzero(finite)[0]
            state[rows, :3] = w[rows]
    cat = lambda parts, like: np.concatenate(parts, axis=0) if parts else like  # noqa: E731
    xyz, desc, node = cat(xyz, out["xyz"]), cat(desc, out["desc"]), cat(node, out["node"])
    row, n_opt = cat(row, out["row"]), cat(n_opt, out["n_opt"])
    total = int(xyz.shape[0])
    out.update(n_total=total, n_nonfinite=n_nonfinite, status=PRS_OK)
    if out_stride is None:
        return out
    k = min(total, int(out_stride))
    out.update(n_out=k, xyz=xyz[:k], desc=desc[:k], node=node[:k], row=row[:k], n_opt=n_opt[:k],
               status=PRS_ERR_CAPACITY if total > int(out_stride) else PRS_OK)
    b = empty_bounds()
    if k:
        v = xyz[:k, :3] + np.float32(0.0)  # -0 becomes +0: min and max have one answer whatever the order
        b = np.concatenate([v.min(axis=0), v.max(axis=0)]).astype(np.float32)
    out["bounds"] = b
    return out


def host_route(archive_maps, live_map, graph_X, p):
    """the route the device call replaces, for tools/bench_world_map.py and the chain test: archive_maps is a list of (node, dict as
    ops.MapArchive.slot_of returns it) in node order, live_map (node, dict(coords, n_opt, inlier, n_points)) or None -> xyz [n, 4]"""
    parts = []
    items = list(archive_maps) + ([live_map] if live_map is not None else [])
    for n, m in sorted(items, key=lambda it: it[0]):
        np_ = int(m["n_points"])
        c = np.asarray(m["coords"], np.float32)[:np_]
        w = world_rows(graph_X[n], c)
        keep = np.isfinite(w).all(axis=1) & (np.asarray(m["n_opt"])[:np_].astype(np.uint32) >= np.uint32(p["min_n_opt"]))
        if p["require_inlier"]:
            keep &= np.asarray(m["inlier"])[:np_] != 0
        parts.append(np.concatenate([w[keep], c[keep, 3:4]], axis=1))
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, 4), np.float32)
