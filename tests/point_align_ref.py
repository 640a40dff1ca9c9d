"""CPU restatements of the loop aligner (include/proslam_hip.h, prs_point_align_batch; csrc/point_align.hip).

`align` is the float32 restatement in the kernel's operation order: the per-correspondence terms element by element, the lane
sums of correspondences k = lane + 64 j in ascending j, the butterfly over the 64 lanes, the camera-frame assembly, the rotation
with separate multiplies and adds, and the checker's `gn_step` (bit for bit the device's prs::gn_step).  `align_f64` is the
independent check: the Jacobian J = R [I | -2 [p]x] built per correspondence in float64, summed directly, solved with numpy.
"""
import math

import numpy as np

from oracle import binding as ob

f32 = np.float32
CLAMP, SATURATED = 0, 1
WARN_NO_MATCHES, ERR_RANGE = 2, -4
_SUMS = 18


def params(robustifier=CLAMP, chi_threshold=3.0, damping=0.0, max_iterations=100, min_num_inliers=10, min_num_correspondences=0,
           relocalize_min_inliers=0, relocalize_min_inliers_ratio=0.0, relocalize_max_chi_inliers=math.inf, linearize_only=0):
    return dict(robustifier=robustifier, chi_threshold=chi_threshold, damping=damping, max_iterations=max_iterations,
                min_num_inliers=min_num_inliers, min_num_correspondences=min_num_correspondences,
                relocalize_min_inliers=relocalize_min_inliers, relocalize_min_inliers_ratio=relocalize_min_inliers_ratio,
                relocalize_max_chi_inliers=relocalize_max_chi_inliers, linearize_only=linearize_only)


def from_loop_group(loop, **overrides):
    """params() of a configs.py `loop` group (the loop detector's verdict thresholds)"""
    p = params(robustifier=SATURATED if loop["robustifier"] == "saturated" else CLAMP, chi_threshold=loop["chi_threshold"],
               damping=loop["damping"], max_iterations=loop["max_iterations"], min_num_inliers=loop["min_num_inliers"],
               min_num_correspondences=loop["min_num_correspondences"], relocalize_min_inliers=loop["relocalize_min_inliers"],
               relocalize_min_inliers_ratio=loop["relocalize_min_inliers_ratio"],
               relocalize_max_chi_inliers=loop["relocalize_max_chi_inliers"])
    p.update(overrides)
    return p


def _indices(corr):
    corr = np.asarray(corr)
    if corr.dtype.names:
        return corr["fixed_idx"].astype(np.int64), corr["moving_idx"].astype(np.int64)
    corr = corr.reshape(-1, 2) if corr.size else np.zeros((0, 2), np.int64)
    return corr[:, 0].astype(np.int64), corr[:, 1].astype(np.int64)


def linearize(P, X, fixed, moving, corr):
    """one linearisation at X -> dict(H [6, 6], b [6], chi_inliers, chi_total, num_inliers / outliers / invalid, cls [n]: 1 inlier,
    0 outlier, -1 invalid), float32 in the kernel's order"""
    X = np.asarray(X, f32).reshape(4, 4)
    fi, mi = _indices(corr)
    n = len(fi)
    tau = f32(P["chi_threshold"])
    saturated = P["robustifier"] == SATURATED
    with np.errstate(all="ignore"):
        p = np.asarray(moving, f32).reshape(-1, 3)[mi] if n else np.zeros((0, 3), f32)
        f = np.asarray(fixed, f32).reshape(-1, 3)[fi] if n else np.zeros((0, 3), f32)
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
        y0 = (X[0, 0] * px + X[0, 1] * py) + X[0, 2] * pz
        y1 = (X[1, 0] * px + X[1, 1] * py) + X[1, 2] * pz
        y2 = (X[2, 0] * px + X[2, 1] * py) + X[2, 2] * pz
        e0 = (y0 + X[0, 3]) - f[:, 0]
        e1 = (y1 + X[1, 3]) - f[:, 1]
        e2 = (y2 + X[2, 3]) - f[:, 2]
        chi = (e0 * e0 + e1 * e1) + e2 * e2
        valid = np.isfinite(chi)
        inlier = valid & (chi <= tau)
        contrib = inlier | (valid & saturated)
        w = np.where(inlier, f32(1.0), f32(1.0) / chi).astype(f32)
        terms = [w, w * y0, w * y1, w * y2, w * (y1 * y1 + y2 * y2), w * (y0 * y0 + y2 * y2), w * (y0 * y0 + y1 * y1),
                 w * (y0 * y1), w * (y0 * y2), w * (y1 * y2), w * e0, w * e1, w * e2,
                 w * (y1 * e2 - y2 * e1), w * (y2 * e0 - y0 * e2), w * (y0 * e1 - y1 * e0),
                 chi, np.where(inlier, chi, tau).astype(f32)]
        masks = [contrib] * 16 + [inlier, valid]
        J = (n + 63) // 64
        T = np.zeros((_SUMS, J * 64), f32)
        M = np.zeros((_SUMS, J * 64), bool)
        for i in range(_SUMS):
            T[i, :n] = terms[i]
            M[i, :n] = masks[i]
        T, M = T.reshape(_SUMS, J, 64), M.reshape(_SUMS, J, 64)
        s = np.zeros((_SUMS, 64), f32)
        for j in range(J):
            s = np.where(M[:, j], s + T[:, j], s)
        lane = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lane ^ m]
    s = s[:, 0]
    H, b = assemble(X, s)
    cls = np.where(valid, np.where(inlier, 1, 0), -1).astype(np.int32)
    return dict(H=H, b=b, chi_inliers=f32(s[16]), chi_total=f32(s[17]), num_inliers=int(inlier.sum()),
                num_outliers=int((valid & ~inlier).sum()), num_invalid=int((~valid).sum()), cls=cls)


def assemble(X, s):
    """the camera-frame system from the 18 sums, rotated: Rt^T H_c Rt, Rt^T b_c (csrc/point_align.hip assemble_system)"""
    Hc = np.zeros((6, 6), f32)
    Hc[0, 0] = Hc[1, 1] = Hc[2, 2] = s[0]
    u0, u1, u2 = f32(2.0) * s[1], f32(2.0) * s[2], f32(2.0) * s[3]
    Hc[0, 4], Hc[0, 5], Hc[1, 3], Hc[1, 5], Hc[2, 3], Hc[2, 4] = u2, -u1, -u2, u0, u1, -u0
    Hc[4, 0], Hc[5, 0], Hc[3, 1], Hc[5, 1], Hc[3, 2], Hc[4, 2] = u2, -u1, -u2, u0, u1, -u0
    Hc[3, 3], Hc[4, 4], Hc[5, 5] = f32(4.0) * s[4], f32(4.0) * s[5], f32(4.0) * s[6]
    d10, d20, d21 = -(f32(4.0) * s[7]), -(f32(4.0) * s[8]), -(f32(4.0) * s[9])
    Hc[4, 3] = Hc[3, 4] = d10
    Hc[5, 3] = Hc[3, 5] = d20
    Hc[5, 4] = Hc[4, 5] = d21
    bc = np.array([s[10], s[11], s[12], f32(2.0) * s[13], f32(2.0) * s[14], f32(2.0) * s[15]], f32)
    R = np.asarray(X, f32).reshape(4, 4)
    Hn = np.zeros((6, 6), f32)
    b = np.zeros(6, f32)
    for r in range(6):
        blk, i = divmod(r, 3)
        Ri0, Ri1, Ri2 = R[0, i], R[1, i], R[2, i]
        Y = Hc[3 * blk:3 * blk + 3]
        for cb in range(2):
            v = [(Ri0 * Y[0, 3 * cb + c] + Ri1 * Y[1, 3 * cb + c]) + Ri2 * Y[2, 3 * cb + c] for c in range(3)]
            for j in range(3):
                Hn[r, 3 * cb + j] = (v[0] * R[0, j] + v[1] * R[1, j]) + v[2] * R[2, j]
        b[r] = (Ri0 * bc[3 * blk] + Ri1 * bc[3 * blk + 1]) + Ri2 * bc[3 * blk + 2]
    H = np.zeros((6, 6), f32)
    for r in range(6):
        for c in range(r + 1):
            H[r, c] = H[c, r] = Hn[r, c]
    return H, b


def gn_step(H, b, damping, X):
    sys = ob.LinearSystem()
    for i in range(36):
        sys.H[i] = H.reshape(36)[i]
    for i in range(6):
        sys.b[i] = b[i]
    return ob.gn_step(sys, damping, X)[0]


def align(P, X0, fixed, moving, corr, n_fixed=None, n_moving=None, match_status=0):
    """the whole call for one pair -> (X [4, 4] float32, result dict with the fields of prs_point_align_result, mask [n] uint8)"""
    X = np.asarray(X0, f32).reshape(4, 4).copy()
    fi, mi = _indices(corr)
    n = len(fi)
    nf = len(np.asarray(fixed).reshape(-1, 3)) if n_fixed is None else n_fixed
    nm = len(np.asarray(moving).reshape(-1, 3)) if n_moving is None else n_moving
    res = dict(H=np.zeros((6, 6), f32), b=np.zeros(6, f32), chi_inliers=f32(0), chi_total=f32(0), num_inliers=0, num_outliers=0,
               num_invalid=0, num_correspondences=n, status=0, accepted=0, iterations=0, warnings=0)
    mask = np.zeros(n, np.uint8)
    if match_status < 0:
        res["warnings"] = match_status
        return X, res, None
    if n and ((fi < 0) | (fi >= nf) | (mi < 0) | (mi >= nm)).any():
        res["warnings"] = ERR_RANGE
        return X, res, None
    run = n > 0 and n >= P["min_num_correspondences"]
    iters = 0 if not run else (1 if P["linearize_only"] else P["max_iterations"])
    lin = None
    for _ in range(iters):
        lin = linearize(P, X, fixed, moving, corr)
        if not P["linearize_only"]:
            X = gn_step(lin["H"], lin["b"], P["damping"], X)
    if lin is not None:
        for k in ("H", "b", "chi_inliers", "chi_total", "num_inliers", "num_outliers", "num_invalid"):
            res[k] = lin[k]
        mask = (lin["cls"] > 0).astype(np.uint8)
    n_in = res["num_inliers"]
    res["iterations"] = iters
    res["status"] = int(iters > 0 and n_in >= P["min_num_inliers"])
    with np.errstate(all="ignore"):
        res["accepted"] = int(bool(res["status"]) and n_in >= P["relocalize_min_inliers"]
                              and f32(n_in) / f32(n) >= f32(P["relocalize_min_inliers_ratio"])
                              and f32(res["chi_inliers"]) / f32(n_in) <= f32(P["relocalize_max_chi_inliers"]))
    if n == 0:
        res["warnings"] = WARN_NO_MATCHES
    return X, res, mask


# ------------------------------------------------------------------------------------------------------------ float64
def linearize_f64(P, X, fixed, moving, corr):
    """H = sum w J^T J, b = sum w J^T e with J = R [I | -2 [p]x] per correspondence, in float64 -> (H, b, chi_inliers, num_inliers)"""
    X = np.asarray(X, np.float64).reshape(4, 4)
    R, t = X[:3, :3], X[:3, 3]
    fi, mi = _indices(corr)
    H, b, chi_in, n_in = np.zeros((6, 6)), np.zeros(6), 0.0, 0
    fixed, moving = np.asarray(fixed, np.float64).reshape(-1, 3), np.asarray(moving, np.float64).reshape(-1, 3)
    for i, m in zip(fi, mi):
        p, f = moving[m], fixed[i]
        e = R @ p + t - f
        chi = float(e @ e)
        if not np.isfinite(chi):
            continue
        if chi <= P["chi_threshold"]:
            w, n_in, chi_in = 1.0, n_in + 1, chi_in + chi
        elif P["robustifier"] == SATURATED:
            w = 1.0 / chi
        else:
            continue
        px = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        J = R @ np.hstack([np.eye(3), -2.0 * px])
        H += w * J.T @ J
        b += w * J.T @ e
    return H, b, chi_in, n_in


def align_f64(P, X0, fixed, moving, corr):
    from ref_pins import gn_step_f64
    X = np.asarray(X0, np.float64).reshape(4, 4).copy()
    for _ in range(P["max_iterations"]):
        H, b, _, _ = linearize_f64(P, X, fixed, moving, corr)
        try:
            if np.linalg.eigvalsh(H + P["damping"] * np.diag(np.diag(H))).min() <= 0:
                break
            X = gn_step_f64(H, b, P["damping"], X)
        except np.linalg.LinAlgError:
            break
    return X


# ------------------------------------------------------------------------------------------------------------ scenarios
# tests/test_loop_closing.cpp: (name, config, query frame, reference frame, max distance, gtest bounds on t2tnq(X * query_in_reference))
KITTI_BOUNDS_01 = (0.2, 0.2, 0.5, 0.01, 0.01, 0.01)
ICL_BOUNDS_01 = (0.05, 0.05, 0.05, 0.01, 0.01, 0.01)
ICL_BOUNDS_50 = (0.1, 0.1, 0.1, 0.05, 0.05, 0.05)


def scenarios(B):
    """the five closures of test_loop_closing.cpp:19-284 -> list of dict(name, config, fixed, fixed_desc, moving, moving_desc,
    max_distance, truth (camera_query_in_reference, float64) or None, bounds).  fixed = the query cloud, moving = the reference."""
    import ref_pins as rp
    k = rp.kitti_fixture(B)
    icl = {i: rp.icl_measurements(B, i) for i in (0, 1, 50)}
    out = [dict(name="kitti_00_00", config="kitti", fixed=k["points_in_camera_00"], fixed_desc=k["desc"][0],
                moving=k["points_in_camera_00"], moving_desc=k["desc"][0], max_distance=25.0, truth=None, bounds=None),
           dict(name="kitti_00_01", config="kitti", fixed=k["points_in_camera_01"], fixed_desc=k["desc"][1],
                moving=k["points_in_camera_00"], moving_desc=k["desc"][0], max_distance=25.0, truth=rp.kitti_relative(1, 0),
                bounds=KITTI_BOUNDS_01)]
    for q, r, dist, bounds in ((1, 0, 35.0, ICL_BOUNDS_01), (50, 0, 75.0, ICL_BOUNDS_50), (50, 1, 75.0, ICL_BOUNDS_50)):
        out.append(dict(name="icl_%02d_%02d" % (r, q), config="icl", fixed=icl[q]["xyz"], fixed_desc=icl[q]["desc"], moving=icl[r]["xyz"],
                        moving_desc=icl[r]["desc"], max_distance=dist, truth=rp.icl_relative(q, r), bounds=bounds))
    return out


def unrelated(B):
    """places that must be rejected: KITTI city 00 / 01 against highway 274, ICL 00 against KITTI city 00"""
    import ref_pins as rp
    k, h, icl = rp.kitti_fixture(B), rp.highway_fixture(B), rp.icl_measurements(B, 0)
    return [dict(name="city00_highway274", config="kitti", fixed=h["points_in_camera_00"], fixed_desc=h["desc"][0],
                 moving=k["points_in_camera_00"], moving_desc=k["desc"][0], max_distance=25.0),
            dict(name="city01_highway274", config="kitti", fixed=h["points_in_camera_00"], fixed_desc=h["desc"][0],
                 moving=k["points_in_camera_01"], moving_desc=k["desc"][1], max_distance=25.0),
            dict(name="icl00_city00", config="icl", fixed=k["points_in_camera_00"], fixed_desc=k["desc"][0], moving=icl["xyz"],
                 moving_desc=icl["desc"], max_distance=35.0)]


def pose_error(X, truth):
    import ref_pins as rp
    return rp.t2tnq(np.asarray(X, np.float64).reshape(4, 4) @ truth)
