"""float64 numpy restatement of the trajectory evaluator's definitions (include/proslam_hip.h, prs_trajectory_eval_batch): alignment by
numpy.linalg.svd with the determinant fix, distances by numpy.cumsum, two-pass standard deviations.  Nothing here follows the kernel's
order of operations or its eigen-solver: it is the yardstick the kernel is compared with, within a tolerance derived from float64 sums
of the same float32 inputs in another order (tests/test_trajectory_gpu.py).  No GPU needed."""
import numpy as np

ALIGN_NONE, ALIGN_FIRST, ALIGN_RIGID = 0, 1, 2
OK, ERR_RANGE = 0, -4
KITTI_LENGTHS = (100, 200, 300, 400, 500, 600, 700, 800)


def to44(poses):
    """[n, 4, 4], [n, 16] or [n, 12] -> float64 [n, 4, 4] of the float32 values the device reads"""
    a = np.asarray(poses, np.float32)
    a = a.reshape(a.shape[0], -1)
    if a.shape[1] == 12:
        a = np.concatenate([a, np.tile(np.array([[0, 0, 0, 1]], np.float32), (a.shape[0], 1))], axis=1)
    return a.astype(np.float64).reshape(-1, 4, 4)


def rel(A, B):
    """A^-1 B with the rigid inverse, batched: [R_a^T R_b | R_a^T (t_b - t_a)]"""
    Rat = np.swapaxes(A[..., :3, :3], -1, -2)
    out = np.zeros(np.broadcast(A, B).shape)
    out[..., :3, :3] = Rat @ B[..., :3, :3]
    out[..., :3, 3] = (Rat @ (B[..., :3, 3] - A[..., :3, 3])[..., None])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def rotation_vector(R):
    """theta = atan2(|v| / 2, (tr R - 1) / 2), v = vee(R - R^T); -> (theta, theta v / |v| with 0 where |v| = 0), batched"""
    v = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    nv = np.linalg.norm(v, axis=-1)
    theta = np.arctan2(0.5 * nv, 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(nv > 0, theta / nv, 0.0)
    return theta, v * s[..., None]


def pair_errors(P, G, i, j):
    """E = (G_i^-1 G_j)^-1 (P_i^-1 P_j) for index arrays i, j -> (|t(E)|, theta, t(E), rotation vector)"""
    E = rel(rel(G[i], G[j]), rel(P[i], P[j]))
    theta, rv = rotation_vector(E[..., :3, :3])
    return np.linalg.norm(E[..., :3, 3], axis=-1), theta, E[..., :3, 3], rv


def rigid_alignment(p, g):
    """the rotation and translation, no scale, minimising sum |g_k - (R p_k + t)|^2 (Umeyama): SVD of the centred cross-covariance with
    the determinant fix, so that R is proper also where the unconstrained optimum is a reflection"""
    cp, cg = p.mean(axis=0), g.mean(axis=0)
    W = (g - cg).T @ (p - cp)
    U, _, Vt = np.linalg.svd(W)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ D @ Vt
    S = np.eye(4)
    S[:3, :3] = R
    S[:3, 3] = cg - R @ cp
    return S


def _zeros(status, n_valid, stride):
    z3, z8 = np.zeros(3), np.zeros(8)
    return dict(status=status, n_valid=n_valid, n_rpe=0, n_kitti=0, S=np.eye(4), path_length=0.0, ate_rmse=0.0, ate_mean=0.0, ate_max=0.0,
                rpe_t_rmse=0.0, rpe_t_mean=0.0, rpe_t_max=0.0, rpe_r_rmse=0.0, rpe_r_mean=0.0, rpe_r_max=0.0, axis_t_mean=z3.copy(),
                axis_t_std=z3.copy(), axis_r_mean=z3.copy(), axis_r_std=z3.copy(), kitti_t=0.0, kitti_r=0.0, kitti_t_len=z8.copy(),
                kitti_r_len=z8.copy(), kitti_n_len=np.zeros(8, np.int32), frame_error=np.full(stride, -1.0), kitti_margin=np.inf)


def evaluate(estimate, ground_truth, n_frames=None, valid=None, align=ALIGN_RIGID, rpe_delta=1, kitti_step=10, lengths=KITTI_LENGTHS):
    """one sequence.  estimate, ground_truth: [frame_stride] poses (rows from n_frames on are never read); -> dict of the fields of
    prs_trajectory_result plus frame_error (float64 [frame_stride]) and kitti_margin: the smallest distance of a selected dist[last]
    or dist[last - 1] from its threshold (inf without subsequences)"""
    P, G = to44(estimate), to44(ground_truth)
    stride = P.shape[0]
    nf = stride if n_frames is None else int(n_frames)
    n = min(max(nf, 0), stride)
    ok = np.ones(n, bool) if valid is None else np.asarray(valid).reshape(-1)[:n] != 0
    rows = np.flatnonzero(ok)
    n_valid = int(rows.size)
    if nf < 0:
        return _zeros(ERR_RANGE, 0, stride)
    if (align == ALIGN_RIGID and n_valid < 3) or (align == ALIGN_FIRST and n_valid < 1):
        return _zeros(ERR_RANGE, n_valid, stride)
    out = _zeros(OK, n_valid, stride)
    tp, tg = P[:n, :3, 3], G[:n, :3, 3]

    if align == ALIGN_RIGID:
        S = rigid_alignment(tp[rows], tg[rows])
    elif align == ALIGN_FIRST:
        f = rows[0]
        S = np.eye(4)
        S[:3, :3] = G[f, :3, :3] @ P[f, :3, :3].T
        S[:3, 3] = G[f, :3, 3] - S[:3, :3] @ P[f, :3, 3]
    else:
        S = np.eye(4)
    out["S"] = S

    both = np.flatnonzero(ok[1:] & ok[:-1]) + 1 if n > 1 else np.zeros(0, int)
    out["path_length"] = float(np.linalg.norm(tg[both] - tg[both - 1], axis=1).sum())

    if n_valid:
        e = np.linalg.norm(tg[rows] - (tp[rows] @ S[:3, :3].T + S[:3, 3]), axis=1)
        out["frame_error"][rows] = e
        out["ate_rmse"], out["ate_mean"], out["ate_max"] = float(np.sqrt(np.mean(e * e))), float(e.mean()), float(e.max())

    if rpe_delta < n:
        k = np.arange(n - rpe_delta)
        k = k[ok[k] & ok[k + rpe_delta]]
        if k.size:
            te, th, tv, rv = pair_errors(P, G, k, k + rpe_delta)
            out["n_rpe"] = int(k.size)
            out["rpe_t_rmse"], out["rpe_t_mean"], out["rpe_t_max"] = float(np.sqrt(np.mean(te * te))), float(te.mean()), float(te.max())
            out["rpe_r_rmse"], out["rpe_r_mean"], out["rpe_r_max"] = float(np.sqrt(np.mean(th * th))), float(th.mean()), float(th.max())
            at, ar = np.abs(tv), np.degrees(np.abs(rv))
            out["axis_t_mean"], out["axis_t_std"] = at.mean(axis=0), at.std(axis=0)
            out["axis_r_mean"], out["axis_r_std"] = ar.mean(axis=0), ar.std(axis=0)

    if kitti_step > 0 and n > 0 and n_valid == n:
        dist = np.concatenate([[0.0], np.cumsum(np.linalg.norm(tg[1:] - tg[:-1], axis=1))])
        sum_t = sum_r = 0.0
        margin = np.inf
        for li, length in enumerate(lengths):
            L = float(np.float32(length))
            firsts, lasts = [], []
            for first in range(0, n, kitti_step):
                limit = dist[first] + L
                beyond = np.flatnonzero(dist[first:] > limit)  # the devkit's scan: the first index past the length
                if beyond.size:
                    last = first + int(beyond[0])
                    firsts.append(first)
                    lasts.append(last)
                    margin = min(margin, abs(dist[last] - limit), abs(dist[last - 1] - limit))
            if firsts:
                te, th, _, _ = pair_errors(P, G, np.array(firsts), np.array(lasts))
                out["kitti_n_len"][li] = len(firsts)
                out["kitti_t_len"][li], out["kitti_r_len"][li] = float((te / L).mean()), float((th / L).mean())
                sum_t += float((te / L).sum())
                sum_r += float((th / L).sum())
        out["n_kitti"] = int(out["kitti_n_len"].sum())
        if out["n_kitti"]:
            out["kitti_t"], out["kitti_r"] = sum_t / out["n_kitti"], sum_r / out["n_kitti"]
        out["kitti_margin"] = margin
    return out
