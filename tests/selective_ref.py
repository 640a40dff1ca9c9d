"""CPU restatement of IntensityFeatureExtractorSelective_ (sensor_processing/feature_extractors/
intensity_feature_extractor_selective.cpp:62-200, intensity_feature_extractor_base.cpp:56-85) with cv::GFTTDetector and
cv::ORB::compute restated from OpenCV's published algorithms.  TEST INFRASTRUCTURE ONLY: the checker of
prs_extract_features_selective*.  Float32 wherever the device computes in float32, in the same operation order, so the
corner responses are bit-equal.

GFTT on one 8-bit image with a 0/1 mask M (goodFeaturesToTrack, blockSize 3, no Harris, quality 0.01):
  Sobel 3x3 (reflect-101) as exact integers, times 1/(4*3*255) in float; products; unnormalised 3x3 box sums (reflect-101),
  row sums then column sums, each ((l + c) + r); eig = (a + c) - sqrt((a - c)^2 + b^2) with a = Sxx/2, b = Sxy, c = Syy/2;
  maxVal over M only; eig := 0 where not eig > float(0.01 * maxVal); 3x3 max dilation; candidates 1 <= y <= rows-2,
  1 <= x <= cols-2, M != 0, eig != 0, eig == dilated; sorted by eig descending, ties by pixel address descending (OpenCV
  >= 3.4 greaterThanPtr: the build's choice, the reference's pins do not decide it); greedy min-distance acceptance
  (dx^2 + dy^2 < minDistance^2 rejects), at most maxCorners.
"""
import numpy as np

from oracle import binding_features as of

BORDER = 31          # cv::ORB edgeThreshold
BASE_RADIUS = 10     # selective.cpp:67
SOBEL_SCALE = np.float32(1.0 / (4 * 3 * 255))
QUALITY = 0.01


def _reflect101(a, pad):
    return np.pad(a, pad, mode="reflect")


def min_eigen(image):
    """cornerMinEigenVal(image, blockSize 3, ksize 3) in float32 -> [rows, cols]"""
    p = _reflect101(np.asarray(image, np.int32), 1)
    # exact integer Sobel: dx = [1 2 1]^T [-1 0 1], dy = [-1 0 1]^T [1 2 1]
    h = p[:, 2:] - p[:, :-2]
    sx = h[:-2] + 2 * h[1:-1] + h[2:]
    v = p[2:, :] - p[:-2, :]
    sy = v[:, :-2] + 2 * v[:, 1:-1] + v[:, 2:]
    dx = sx.astype(np.float32) * SOBEL_SCALE
    dy = sy.astype(np.float32) * SOBEL_SCALE
    prods = [dx * dx, dx * dy, dy * dy]
    sums = []
    for q in prods:
        qp = _reflect101(q, 1)
        r = (qp[:, :-2] + qp[:, 1:-1]) + qp[:, 2:]
        sums.append((r[:-2] + r[1:-1]) + r[2:])
    a = sums[0] * np.float32(0.5)
    b = sums[1]
    c = sums[2] * np.float32(0.5)
    d = a - c
    return (a + c) - np.sqrt(d * d + b * b)


def candidates(image, mask, eig=None):
    """goodFeaturesToTrack's candidates before the distance test -> (ys, xs) sorted by response desc, pixel address desc"""
    img = np.asarray(image, np.uint8)
    rows, cols = img.shape
    m = np.ones((rows, cols), bool) if mask is None else np.asarray(mask) != 0
    e = min_eigen(img) if eig is None else eig.copy()
    max_val = float(e[m].max()) if m.any() else 0.0
    thr = np.float32(max_val * QUALITY)
    e[~(e > thr)] = 0
    ep = np.pad(e, 1, mode="edge")
    dil = ep[1:-1, 1:-1].copy()
    for oy in (0, 1, 2):
        for ox in (0, 1, 2):
            dil = np.maximum(dil, ep[oy:oy + rows, ox:ox + cols])
    cand = np.zeros((rows, cols), bool)
    cand[1:-1, 1:-1] = True
    cand &= m & (e != 0) & (e == dil)
    ys, xs = np.nonzero(cand)
    addr = ys.astype(np.int64) * cols + xs
    vals = e[ys, xs]
    order = np.lexsort((-addr, -vals.astype(np.float64)))
    return ys[order], xs[order]


def gftt(image, mask, max_corners, min_distance, eig=None):
    """-> [n, 2] int (x, y) in acceptance order"""
    rows, cols = np.asarray(image).shape
    ys, xs = candidates(image, mask, eig)
    out = []
    md2 = min_distance * min_distance
    if min_distance >= 1:
        cell = int(min_distance)
        gw = (cols + cell - 1) // cell
        gh = (rows + cell - 1) // cell
        grid = [[] for _ in range(gw * gh)]
        for y, x in zip(ys.tolist(), xs.tolist()):
            gx, gy = x // cell, y // cell
            good = True
            for cy in range(max(gy - 1, 0), min(gy + 2, gh)):
                for cx in range(max(gx - 1, 0), min(gx + 2, gw)):
                    for (px, py) in grid[cy * gw + cx]:
                        if (x - px) ** 2 + (y - py) ** 2 < md2:
                            good = False
                            break
                    if not good:
                        break
                if not good:
                    break
            if good:
                grid[gy * gw + gx].append((x, y))
                out.append((x, y))
                if len(out) == max_corners:
                    break
    else:
        out = list(zip(xs.tolist(), ys.tolist()))[:max_corners]
    return np.array(out, np.int64).reshape(-1, 2)


def round_half_away(v):
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def tracking_mask(rows, cols, projections, radius, full_left=False, full_right=False):
    """selective.cpp:64-150: 1 inside the union of the projections' rectangles (the seeding mask is its complement)"""
    t = np.zeros((rows, cols), np.uint8)
    r = int(radius) + BASE_RADIUS
    uv = np.asarray(projections, np.float32).reshape(-1, 2)
    for col, row in zip(round_half_away(uv[:, 0]).tolist(), round_half_away(uv[:, 1]).tolist()):
        tl_row = max(row - r, 0)
        height = min(2 * r, rows - tl_row)
        if full_left and full_right:
            c0, c1 = 0, cols
        elif full_left:
            c0, c1 = 0, col
        elif full_right:
            c0, c1 = col, cols
        else:
            c0 = max(col - r, 0)
            c1 = c0 + min(2 * r, cols - c0)
        t[tl_row:tl_row + height, c0:c1] = 1
    return t


def describe(image, xy):
    """cv::ORB::compute on integer keypoints with angle -1: border filter (order kept), then 256 comparisons of the
    7x7 fixed-point Gaussian -> (uv [n,2] f32, intensity [n] f32, desc [n,32] u8)"""
    img = np.asarray(image, np.uint8)
    rows, cols = img.shape
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    keep = (xy[:, 0] >= BORDER) & (xy[:, 0] < cols - BORDER) & (xy[:, 1] >= BORDER) & (xy[:, 1] < rows - BORDER)
    xy = xy[keep]
    blur = of.gaussian_blur7(img).astype(np.int32)
    pat = of.orb_pattern().astype(np.int64)
    x, y = xy[:, 0:1], xy[:, 1:2]
    bits = blur[y + pat[None, :, 1], x + pat[None, :, 0]] < blur[y + pat[None, :, 3], x + pat[None, :, 2]]
    desc = np.packbits(bits.astype(np.uint8), axis=1, bitorder="little")
    uv = xy.astype(np.float32)
    inten = img[xy[:, 1], xy[:, 0]].astype(np.float32)
    return uv, inten, desc.reshape(-1, 32)


def extract(image, target, bin_width, projections=None, radius=0, full_left=False, full_right=False,
            seeding_when_tracking=True, external_mask=None, eig=None):
    """IntensityFeatureExtractorSelective_::compute for one image.  projections: [n, 2] (u, v) or None / empty = seeding.
    -> (uv, intensity, desc) in the reference's order (tracking keypoints, then the seeded ones)"""
    img = np.asarray(image, np.uint8)
    rows, cols = img.shape
    e = min_eigen(img) if eig is None else eig
    if projections is not None and len(projections) > 0:
        t = tracking_mask(rows, cols, projections, radius, full_left, full_right)
        xy = gftt(img, t, target, bin_width, eig=e)
        if seeding_when_tracking:
            xy = np.concatenate([xy, gftt(img, 1 - t, target, bin_width, eig=e)])
    else:
        xy = gftt(img, external_mask, target, bin_width, eig=e)
    return describe(img, xy)
