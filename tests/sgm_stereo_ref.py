"""numpy restatement of the semi-global dense stereo stage (prs_sgm_stereo_batch_run; the rule is stated in include/proslam_hip.h,
BUILD-DEFINED).  It builds the whole raw cost volume C [rows, cols, n], runs every path as a loop along its line, vectorised over the
other axis and over the disparities (a diagonal step reads the previous row shifted by dx), sums the path costs into S and takes the
winner, the uniqueness test, the left-right check (the right image's costs read from the left volume), the sub-pixel part and the
depth exactly as dense_stereo_ref does on its box sums.  It knows nothing of the kernels' lines, lanes or chunks."""
import numpy as np

from dense_stereo_ref import NONE, PRS_ERR_RANGE, PRS_OK, census, winner  # noqa: F401

F = np.float32
BIG = 1 << 20  # stands for a path cost that is left out of a minimum
PATHS = {4: ((0, 1), (0, -1), (1, 0), (-1, 0)), 8: ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))}


def params(bf, n_disparities=128, min_disparity=0, p1=10, p2=120, n_paths=8, uniqueness_percent=10, lr_max_diff=1):
    return dict(bf=F(bf), n_disparities=int(n_disparities), min_disparity=int(min_disparity), p1=int(p1), p2=int(p2), n_paths=int(n_paths),
                uniqueness_percent=int(uniqueness_percent), lr_max_diff=int(lr_max_diff))


def raw_cost(cL, cR, ds):
    """C [rows, cols, n] int32: popcount(cL(y, x) ^ cR(y, max(x - d_i, 0))), for every i, admissible or not"""
    xs = np.arange(cL.shape[1])
    return np.stack([np.bitwise_count(cL ^ cR[:, np.maximum(xs - d, 0)]) for d in ds], axis=-1).astype(np.int32)


def step(Cp, Lq, inside, p1, p2):
    """the path costs [..., n] of pixels p from those of their predecessors q; inside [...]: q is in the image"""
    m = Lq.min(axis=-1, keepdims=True)
    pad = np.full(Lq.shape[:-1] + (1,), BIG, Lq.dtype)
    below = np.concatenate([pad, Lq[..., :-1]], axis=-1) + p1
    above = np.concatenate([Lq[..., 1:], pad], axis=-1) + p1
    L = Cp + np.minimum(np.minimum(Lq, m + p2), np.minimum(below, above)) - m
    return np.where(inside[..., None], L, Cp)


def path_cost(C, dy, dx, p1, p2):
    """L_r [rows, cols, n] int32 of the path that travels in direction (dy, dx)"""
    rows, cols, _ = C.shape
    L = np.empty_like(C)
    if dy == 0:
        for x in (range(cols) if dx > 0 else range(cols - 1, -1, -1)):
            q = x - dx
            L[:, x] = step(C[:, x], L[:, q], np.full(rows, True), p1, p2) if 0 <= q < cols else C[:, x]
        return L
    xq = np.arange(cols) - dx
    inside = (xq >= 0) & (xq < cols)
    xq = np.clip(xq, 0, cols - 1)
    for y in (range(rows) if dy > 0 else range(rows - 1, -1, -1)):
        q = y - dy
        L[y] = step(C[y], L[q][xq], inside, p1, p2) if 0 <= q < rows else C[y]
    return L


def aggregate(C, n_paths, p1, p2):
    """S [rows, cols, n] int32, and the largest path cost met"""
    S, top = np.zeros_like(C), 0
    for dy, dx in PATHS[n_paths]:
        L = path_cost(C, dy, dx, p1, p2)
        S += L
        top = max(top, int(L.max()))
    return S, top


def sgm_stereo_image(left, right, p, details=False):
    """one rectified pair -> dict(disparity, depth float32 [rows, cols], n_valid); details adds S [rows, cols, n] and max_path_cost"""
    n, d0, q, lr = p["n_disparities"], p["min_disparity"], p["uniqueness_percent"], p["lr_max_diff"]
    cL, cR = census(left), census(right)
    rows, cols = cL.shape
    ds = d0 + np.arange(n)
    us = np.arange(cols)
    S, top = aggregate(raw_cost(cL, cR, ds), p["n_paths"], p["p1"], p["p2"])
    assert S.max() < NONE
    A = np.ascontiguousarray(S.transpose(2, 0, 1)).astype(np.uint16)  # [n, rows, cols], as dense_stereo_ref.winner takes it
    adm_l = (us[None, :] - ds[:, None] >= 0)[:, None, :]
    best, a0, a2 = winner(A, adm_l)
    keep = best >= 0
    if q > 0:
        keep &= (a2 >= NONE) | (100 * a0 < (100 - q) * a2)
    i = np.maximum(best, 0)
    dstar = d0 + i
    if lr >= 0:
        adm_r = (us[None, :] + ds[:, None] <= cols - 1)[:, None, :]
        A_r = np.stack([A[k][:, np.minimum(us + d, cols - 1)] for k, d in enumerate(ds)])  # S_R(y, x, i) = S(y, x + d_i, i)
        best_r, _, _ = winner(A_r, adm_r)
        xr = np.clip(us[None, :] - dstar, 0, cols - 1)  # inside already where the pixel has a winner
        ir = np.take_along_axis(best_r, xr, 1)
        keep &= (ir >= 0) & (np.abs(ir - i) <= lr)
    am = np.take_along_axis(A, np.maximum(i - 1, 0)[None], 0)[0].astype(np.int64)
    ap = np.take_along_axis(A, np.minimum(i + 1, n - 1)[None], 0)[0].astype(np.int64)
    den = (am + ap) - 2 * a0
    sub = (i >= 1) & (i + 1 <= n - 1) & (us[None, :] - (dstar + 1) >= 0) & (den > 0) & (best >= 0)
    delta = np.zeros((rows, cols), F)
    delta[sub] = (am - ap)[sub].astype(F) / (2 * den)[sub].astype(F)
    s = dstar.astype(F) + delta
    valid = keep & (s > 0)
    disparity = np.where(valid, s, F(0)).astype(F)
    depth = np.zeros((rows, cols), F)
    depth[valid] = p["bf"] / s[valid]
    out = dict(disparity=disparity, depth=depth, n_valid=int(valid.sum()))
    if details:
        out.update(S=S, max_path_cost=top)
    return out


def sgm_stereo(left, right, n_images, p):
    """one sequence: left, right [frames, rows, cols] uint8 -> dict(status, results: a list with a dict per image, None for the images
    that are not touched)"""
    frames = left.shape[0]
    n = frames if n_images is None else int(n_images)
    if n < 0 or n > frames:
        return dict(status=PRS_ERR_RANGE, results=[None] * frames)
    return dict(status=PRS_OK, results=[sgm_stereo_image(left[f], right[f], p) if f < n else None for f in range(frames)])
