"""The closure merger's rule (include/proslam_hip.h, "Closure merger": BUILD-DEFINED, fitted to the two pins of the reference's
tests/test_mergers.cpp:174-246) in numpy float32, every expression written out term by term in the order the kernel evaluates it
(csrc/closure_merge.hip, built with -ffp-contract=off), so that the two agree bit for bit.  Shared by the CPU and the GPU tests."""
import numpy as np

XYZ, UVD = 0, 1
OK, ERR_CAPACITY, ERR_RANGE, ERR_SCENE_FULL, ERR_DUPLICATE = 0, -2, -4, -8, -9
f32 = np.float32

CORR_DTYPE = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])


def params(kind=UVD, enable_binning=1, row_bins=10, col_bins=30, rows=480, cols=640, K=(481.2, -481.0, 319.5, 239.5),
           max_distance2=0.25, max_response=50.0, target=200):
    return dict(measurement_kind=kind, enable_binning=enable_binning, number_of_row_bins=row_bins, number_of_col_bins=col_bins,
                canvas_rows=rows, canvas_cols=cols, fx=f32(K[0]), fy=f32(K[1]), cx=f32(K[2]), cy=f32(K[3]),
                maximum_distance_geometry_squared=f32(max_distance2), maximum_response=f32(max_response),
                target_number_of_merges=int(target))


def make_scene(capacity, xyz, desc, with_stats=True):
    """a scene of len(xyz) landmarks in arrays of `capacity` rows (rows past n_points carry a pattern: they must not leak)"""
    n = len(xyz)
    s = dict(coords=np.zeros((capacity, 4), f32), desc=np.zeros((capacity, 32), np.uint8), n_points=n)
    s["coords"][:n, :3] = xyz
    s["desc"][:n] = desc
    if with_stats:
        s["state"] = np.zeros((capacity, 4), f32)
        s["state"][:n, :3] = xyz
        s["covariance"] = np.zeros((capacity, 9), f32)
        s["n_opt"] = np.zeros(capacity, np.uint32)
        s["inlier"] = np.zeros(capacity, np.uint8)
        s["n_meas"] = np.zeros(capacity, np.uint32)
    return s


def copy_scene(s):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def scenes_equal(a, b):
    """byte identity of every array (whole capacity) and of the count"""
    if set(a) != set(b) or a["n_points"] != b["n_points"]:
        return False
    return all(a[k].tobytes() == b[k].tobytes() for k in a if k != "n_points")


def se3_inverse(T):
    T = np.asarray(T, f32).reshape(4, 4)
    Ti = np.zeros((4, 4), f32)
    tx, ty, tz = T[0, 3], T[1, 3], T[2, 3]
    for i in range(3):
        r0, r1, r2 = T[0, i], T[1, i], T[2, i]
        Ti[i, 0], Ti[i, 1], Ti[i, 2] = r0, r1, r2
        Ti[i, 3] = -((r0 * tx + r1 * ty) + r2 * tz)
    Ti[3, 3] = 1.0
    return Ti


def apply_rows(T, p):
    """T * p for [n, 3] points: ((t0 x + t1 y) + t2 z) + t3 per row"""
    T = np.asarray(T, f32).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], axis=1).astype(f32)


def measurement_points(P, z):
    """-> (points in the measurement frame [n, 3], valid [n])"""
    z = np.asarray(z, f32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        if P["measurement_kind"] == UVD:
            d = z[:, 2]
            p = np.stack([(z[:, 0] - P["cx"]) / P["fx"] * d, (z[:, 1] - P["cy"]) / P["fy"] * d, d], axis=1).astype(f32)
            valid = np.isfinite(p).all(axis=1) & (d > 0)
        else:
            p = z[:, :3].copy()
            valid = np.isfinite(p).all(axis=1)
    return p, valid


def _round(x):
    """std::round of a float32 >= 0: half away from zero (x - floor(x) is exact)"""
    fl = np.floor(x)
    return int(fl) + (1 if f32(x - fl) >= f32(0.5) else 0)


def bins_of(P, z, p):
    """-> bin index per measurement, -1 = unbinned"""
    z = np.asarray(z, f32).reshape(-1, 4)
    n = len(z)
    with np.errstate(all="ignore"):
        if P["measurement_kind"] == UVD:
            u, v = z[:, 0], z[:, 1]
            front = np.ones(n, bool)
        else:
            u = P["fx"] * p[:, 0] / p[:, 2] + P["cx"]
            v = P["fy"] * p[:, 1] / p[:, 2] + P["cy"]
            front = p[:, 2] > 0
        on = front & (u >= 0) & (u < f32(P["canvas_cols"])) & (v >= 0) & (v < f32(P["canvas_rows"]))
        row_w = f32(P["canvas_rows"]) / f32(P["number_of_row_bins"])
        col_w = f32(P["canvas_cols"]) / f32(P["number_of_col_bins"])
        nbc = P["number_of_col_bins"] + 2
        out = np.full(n, -1, np.int64)
        for i in np.nonzero(on)[0]:
            out[i] = _round(f32(v[i] / row_w)) * nbc + _round(f32(u[i] / col_w))
    return out


def closure_merge(P, scene, measurement, measurement_desc, corr, transform, scene_in_world=None, transform_is_scene_in_measurement=0,
                  corr_from_aligner=0, n_measured=None, n_corr=None, gate_accepted=None, info=None):
    """-> (scene after, (n_merged, n_added, status)).  `scene` is not modified.  measurement [stride, 4], corr CORR_DTYPE [stride];
    n_measured / n_corr default to the array lengths (pass them to exercise the count checks).  info (a dict) receives the sets."""
    S = copy_scene(scene)
    cap = S["coords"].shape[0]
    z = np.asarray(measurement, f32).reshape(-1, 4)
    zd = np.asarray(measurement_desc, np.uint8).reshape(-1, 32)
    n_meas = len(z) if n_measured is None else int(n_measured)
    n_c = len(corr) if n_corr is None else int(n_corr)
    n_points = int(S["n_points"])
    if gate_accepted is not None and not gate_accepted:
        return S, (0, 0, OK)
    if n_points < 0 or n_points > cap or n_meas < 0 or n_c < 0:
        return S, (0, 0, ERR_RANGE)
    if n_meas > len(z) or n_c > len(corr):
        return S, (0, 0, ERR_CAPACITY)
    z, zd = z[:n_meas], zd[:n_meas]
    si = np.asarray(corr["moving_idx" if corr_from_aligner else "fixed_idx"][:n_c], np.int64)
    mi = np.asarray(corr["fixed_idx" if corr_from_aligner else "moving_idx"][:n_c], np.int64)
    resp = np.asarray(corr["response"][:n_c], f32)
    seen = set()
    for s, m in zip(si, mi):  # the first fault in vector order
        if s < 0 or s >= n_points or m < 0 or m >= n_meas:
            return S, (0, 0, ERR_RANGE)
        if s in seen:
            return S, (0, 0, ERR_DUPLICATE)
        seen.add(int(s))
    T = np.asarray(transform, f32).reshape(4, 4)
    if transform_is_scene_in_measurement:
        T = se3_inverse(T)
    W = None if scene_in_world is None else np.asarray(scene_in_world, f32).reshape(4, 4)
    p, valid = measurement_points(P, z)
    q = apply_rows(T, p)
    # ---- merge ----
    merged_meas = np.zeros(n_meas, bool)
    n_merged = 0
    with np.errstate(all="ignore"):
        for s, m, r in zip(si, mi, resp):
            ok = False
            if valid[m] and not (r >= P["maximum_response"]):
                c = S["coords"][s, :3]
                dx, dy, dz = c[0] - q[m, 0], c[1] - q[m, 1], c[2] - q[m, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                ok = bool(d2 < P["maximum_distance_geometry_squared"])
            if ok:
                S["coords"][s, :3] = f32(0.5) * (S["coords"][s, :3] + q[m])
                S["desc"][s] = zd[m]
                merged_meas[m] = True
                n_merged += 1
                if "n_opt" in S:
                    S["n_opt"][s] += 1
                if "state" in S:
                    S["state"][s, :3] = apply_rows(W, S["coords"][s:s + 1, :3])[0]
                    S["state"][s, 3] = 0
            if "inlier" in S:
                S["inlier"][s] = 1 if ok else 0
    # ---- how many to add, and which ----
    target = P["target_number_of_merges"]
    n_to_add = max(min(target - n_merged, n_meas - n_merged), 0) if n_merged < target else 0
    cand = valid & ~merged_meas
    chosen = np.zeros(n_meas, bool)
    pass1 = np.zeros(n_meas, bool)
    n_winners = 0
    if cand.sum() <= n_to_add:
        chosen = cand.copy()
    elif not P["enable_binning"]:
        chosen[np.nonzero(cand)[0][:n_to_add]] = True
    else:
        b = bins_of(P, z, p)
        blocked = set(int(x) for x in b[merged_meas & (b >= 0)])
        best = {}
        for i in np.nonzero(cand & (b >= 0))[0]:
            if int(b[i]) in blocked:
                continue
            key = (p[i, 2], int(i))
            if int(b[i]) not in best or key < best[int(b[i])]:
                best[int(b[i])] = key
        winners = sorted(k[1] for k in best.values())
        n_winners = len(winners)
        pass1[winners[:n_to_add]] = True
        chosen = pass1.copy()
        rest = n_to_add - int(pass1.sum())
        if rest > 0:
            chosen[np.nonzero(cand & ~pass1)[0][:rest]] = True
    n_added = int(chosen.sum())
    if info is not None:
        info.update(merged=np.nonzero(merged_meas)[0], added=np.nonzero(chosen)[0], pass1=np.nonzero(pass1)[0], n_winners=n_winners, n_to_add=n_to_add,
                    bins=bins_of(P, z, p) if P["enable_binning"] else None)
    if n_points + n_added > cap:
        return S, (n_merged, 0, ERR_SCENE_FULL)
    # ---- append in ascending measurement index ----
    for k, m in enumerate(np.nonzero(chosen)[0]):
        r = n_points + k
        S["coords"][r, :3], S["coords"][r, 3] = q[m], 0
        S["desc"][r] = zd[m]
        if "state" in S:
            S["state"][r, :3], S["state"][r, 3] = apply_rows(W, q[m:m + 1])[0], 0
        if "covariance" in S:
            S["covariance"][r] = np.eye(3, dtype=f32).reshape(9)
        if "n_opt" in S:
            S["n_opt"][r] = 0
        if "inlier" in S:
            S["inlier"][r] = 1
        if "n_meas" in S:
            S["n_meas"][r] = 0
    S["n_points"] = n_points + n_added
    return S, (n_merged, n_added, OK)
