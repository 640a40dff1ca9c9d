"""numpy restatement of the dense stereo stage (prs_dense_stereo_batch_run; the rule is stated in include/proslam_hip.h,
BUILD-DEFINED).  It builds the whole cost volume with clipped index arrays and knows nothing of the kernels' tiles: census words of a
9 x 7 window, Hamming costs, a clamped box sum, the winner over the admissible disparities with its runner-up two or more away, the
integer uniqueness test, the left-right check, one float32 division and one addition for the sub-pixel part, one division for the
depth."""
import numpy as np

F = np.float32
PRS_OK, PRS_ERR_RANGE = 0, -4
NONE = 0xffff  # "no such cost": above every sum of costs


def params(bf, n_disparities=128, min_disparity=0, aggregation_radius=3, uniqueness_percent=10, lr_max_diff=1):
    return dict(bf=F(bf), n_disparities=int(n_disparities), min_disparity=int(min_disparity), aggregation_radius=int(aggregation_radius),
                uniqueness_percent=int(uniqueness_percent), lr_max_diff=int(lr_max_diff))


def census(image):
    """[rows, cols] uint8 -> uint64: one bit per offset of the 9 wide x 7 tall window but the centre, I(y + dy, x + dx) < I(y, x) at
    clamped coordinates"""
    I = np.asarray(image, np.uint8)
    rows, cols = I.shape
    ys, xs = np.arange(rows), np.arange(cols)
    out = np.zeros((rows, cols), np.uint64)
    bit = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            n = I[np.clip(ys + dy, 0, rows - 1)][:, np.clip(xs + dx, 0, cols - 1)]
            out |= (n < I).astype(np.uint64) << np.uint64(bit)
            bit += 1
    assert bit == 62
    return out


def aggregated(c_ref, c_other, ds, sign, r):
    """A[i][v][u]: the box sum of radius r, at clamped coordinates, of popcount(c_ref(y, x) ^ c_other(y, clamp(x + sign * d_i))); uint16,
    which holds 62 * 15 * 15"""
    rows, cols = c_ref.shape
    ys, xs = np.arange(rows), np.arange(cols)
    A = np.zeros((len(ds), rows, cols), np.uint16)
    for i, d in enumerate(ds):
        C = np.bitwise_count(c_ref ^ c_other[:, np.clip(xs + sign * d, 0, cols - 1)]).astype(np.uint16)
        V = np.zeros_like(C)
        for dy in range(-r, r + 1):
            V += C[np.clip(ys + dy, 0, rows - 1), :]
        for dx in range(-r, r + 1):
            A[i] += V[:, np.clip(xs + dx, 0, cols - 1)]
    return A


def winner(A, admissible):
    """rule 5 -> (i* the index of the winner or -1, A0, A2 or NONE)"""
    n = A.shape[0]
    M = np.where(admissible, A, np.uint16(NONE))
    best = np.argmin(M, axis=0)  # the first of equal costs: the lowest d
    a0 = np.take_along_axis(M, best[None], 0)[0]
    for k in (-1, 0, 1):  # what is left is two or more away from the winner
        np.put_along_axis(M, np.clip(best + k, 0, n - 1)[None], np.uint16(NONE), 0)
    a2 = M.min(axis=0)
    return np.where(a0 < NONE, best, -1), a0.astype(np.int64), a2.astype(np.int64)


def dense_stereo_image(left, right, p):
    """one rectified pair -> dict(disparity, depth float32 [rows, cols], n_valid)"""
    n, d0, r, q, lr = p["n_disparities"], p["min_disparity"], p["aggregation_radius"], p["uniqueness_percent"], p["lr_max_diff"]
    cL, cR = census(left), census(right)
    rows, cols = cL.shape
    ds = d0 + np.arange(n)
    us = np.arange(cols)
    adm_l = (us[None, :] - ds[:, None] >= 0)[:, None, :]
    A = aggregated(cL, cR, ds, -1, r)
    best, a0, a2 = winner(A, adm_l)
    keep = best >= 0
    if q > 0:
        keep &= (a2 >= NONE) | (100 * a0 < (100 - q) * a2)
    i = np.maximum(best, 0)
    dstar = d0 + i
    if lr >= 0:
        adm_r = (us[None, :] + ds[:, None] <= cols - 1)[:, None, :]
        best_r, _, _ = winner(aggregated(cR, cL, ds, +1, r), adm_r)
        xr = np.clip(us[None, :] - dstar, 0, cols - 1)  # inside already where the pixel has a winner
        ir = np.take_along_axis(best_r, xr, 1)
        keep &= (ir >= 0) & (np.abs(ir - i) <= lr)
    # sub-pixel: both neighbours in the range and admissible (for a left pixel: u - (d* + 1) >= 0)
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
    return dict(disparity=disparity, depth=depth, n_valid=int(valid.sum()))


def dense_stereo(left, right, n_images, p):
    """one sequence: left, right [frames, rows, cols] uint8 -> dict(status, results: a list with a dict per image, None for the images
    that are not touched)"""
    frames = left.shape[0]
    n = frames if n_images is None else int(n_images)
    if n < 0 or n > frames:
        return dict(status=PRS_ERR_RANGE, results=[None] * frames)
    return dict(status=PRS_OK, results=[dense_stereo_image(left[f], right[f], p) if f < n else None for f in range(frames)])
