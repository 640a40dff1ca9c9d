"""The CPU checker of the selective extractor (tests/selective_ref.py) against the counts the reference's own gtests assert
(srrg2_proslam/tests/test_feature_extractors.cpp:168-262, KITTI city_left[0]) and on small hand-checkable cases:
the projection rectangles of the four flag combinations, clipping at every border, seeding-when-tracking with its own
budget, an empty tracking mask, the external seeding mask."""
import numpy as np
import pytest

import ref_pins as rp
import selective_ref as sr


@pytest.fixture(scope="module")
def kitti():
    img = rp.kitti_image("left", 0)
    return img, sr.min_eigen(img)


@pytest.mark.parametrize("descriptor", ["ORB-256", "BRIEF-256"])  # both are cv::ORB in the reference's build
def test_reference_counts_on_kitti(kitti, descriptor):
    img, eig = kitti
    seeded, _, _ = sr.extract(img, 100, 10, eig=eig)
    assert len(seeded) == 94
    for radius, expected in ((100, 719), (50, 581), (10, 294), (5, 237)):
        uv, inten, desc = sr.extract(img, 1000, 10, projections=seeded, radius=radius, seeding_when_tracking=False, eig=eig)
        assert len(uv) == expected, radius
        assert desc.shape == (expected, 32) and np.array_equal(inten, img[uv[:, 1].astype(int), uv[:, 0].astype(int)].astype(np.float32))


def test_where_the_mask_applies_decides_the_small_radii(kitti):
    """masking the response map itself (instead of the maximum and the candidates) creates false maxima at the mask edge"""
    img, eig = kitti
    seeded, _, _ = sr.extract(img, 100, 10, eig=eig)
    t = sr.tracking_mask(*img.shape, seeded, 10)
    masked = np.where(t != 0, eig, np.float32(0))
    wrong = sr.describe(img, sr.gftt(img, t, 1000, 10, eig=masked))[0]
    assert len(wrong) != 294


ROWS, COLS = 40, 60


def _rect(m):
    ys, xs = np.nonzero(m)
    return (int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1) if len(ys) else None


@pytest.mark.parametrize("left,right,cols", [(False, False, (10, 30)), (True, False, (0, 20)), (False, True, (20, COLS)), (True, True, (0, COLS))])
def test_rectangle_modes(left, right, cols):
    m = sr.tracking_mask(ROWS, COLS, [(20.0, 15.0)], 0, left, right)  # r = 0 + 10
    assert _rect(m) == (5, 25) + cols
    assert m.sum() == 20 * (cols[1] - cols[0])  # one solid rectangle


def test_rectangles_clipped_at_every_border():
    # top-left: the rectangle starts at 0 and keeps its full 2r extent ([tl, tl + min(2r, size - tl)), selective.cpp:136-143)
    assert _rect(sr.tracking_mask(ROWS, COLS, [(2.0, 3.0)], 0)) == (0, 20, 0, 20)
    # bottom-right: cut at the image
    assert _rect(sr.tracking_mask(ROWS, COLS, [(58.0, 38.0)], 0)) == (28, 40, 48, 60)
    # a radius larger than the image covers it
    assert sr.tracking_mask(ROWS, COLS, [(30.0, 20.0)], 100).all()
    # half-pixel projections round away from zero (std::round)
    assert _rect(sr.tracking_mask(ROWS, COLS, [(20.5, 14.5)], 0)) == (5, 25, 11, 31)
    # left-only at column 0 and right-only at the last column + 0.5 are empty
    assert not sr.tracking_mask(ROWS, COLS, [(0.0, 20.0)], 0, True, False).any()
    assert not sr.tracking_mask(ROWS, COLS, [(59.5, 20.0)], 0, False, True).any()


def _squares(rows=96, cols=160):
    """black image with white 10x10 squares on a 20-px lattice: strong corners at every square corner"""
    img = np.zeros((rows, cols), np.uint8)
    for y in range(6, rows - 16, 20):
        for x in range(6, cols - 16, 20):
            img[y:y + 10, x:x + 10] = 200
    return img


def test_gftt_finds_the_square_corners():
    img = _squares()
    xy = sr.gftt(img, None, 1000, 3)
    assert len(xy) > 0
    # every accepted corner lies at a corner pixel of a square, within one pixel
    for x, y in xy.tolist():
        assert min(abs((x - 6) % 20 - d) for d in (0, 9, 20)) <= 1 and min(abs((y - 6) % 20 - d) for d in (0, 9, 20)) <= 1
    # greedy min distance: no two accepted corners closer than 3
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)
    assert (d2[np.triu_indices(len(xy), 1)] >= 9).all()
    assert len(sr.gftt(img, None, 5, 3)) == 5  # maxCorners


def test_seeding_when_tracking_appends_its_own_budget():
    img = _squares()
    proj = [(40.0, 40.0)]
    t = sr.tracking_mask(*img.shape, proj, 0)
    track = sr.gftt(img, t, 4, 3)
    seed = sr.gftt(img, 1 - t, 4, 3)
    assert len(track) == 4 and len(seed) == 4  # each run fills its own maxCorners
    assert all(t[y, x] for x, y in track.tolist()) and not any(t[y, x] for x, y in seed.tolist())
    uv_off = sr.extract(img, 4, 3, projections=proj, radius=0, seeding_when_tracking=False)[0]
    uv_on = sr.extract(img, 4, 3, projections=proj, radius=0, seeding_when_tracking=True)[0]
    assert np.array_equal(uv_on[:len(uv_off)], uv_off)  # appended behind the tracking keypoints
    assert np.array_equal(uv_on, sr.describe(img, np.concatenate([track, seed]))[0])


def test_empty_tracking_mask():
    img = _squares()
    # full_distance_to_left at column 0: an empty rectangle; the tracking run finds nothing, the seeding run everything
    proj = [(0.0, 40.0)]
    assert len(sr.extract(img, 100, 3, projections=proj, full_left=True, seeding_when_tracking=False)[0]) == 0
    uv = sr.extract(img, 100, 3, projections=proj, full_left=True, seeding_when_tracking=True)[0]
    assert np.array_equal(uv, sr.extract(img, 100, 3)[0])


def test_external_seeding_mask():
    img = _squares()
    mask = np.zeros(img.shape, np.uint8)
    mask[:, :80] = 1
    xy = sr.gftt(img, mask, 1000, 3)
    assert len(xy) > 0 and (xy[:, 0] < 80).all()
    uv = sr.extract(img, 1000, 3, external_mask=mask)[0]
    assert len(uv) > 0 and (uv[:, 0] < 80).all()
    # the external mask is a seeding-mode input only: with projections it is ignored
    proj = [(40.0, 40.0)]
    assert np.array_equal(sr.extract(img, 100, 3, projections=proj, external_mask=mask)[0], sr.extract(img, 100, 3, projections=proj)[0])


def _reflect101_index(n, pad):
    """indices of a row or column padded by `pad` with BORDER_REFLECT_101 (..., 2, 1 | 0, 1, ..., n-1 | n-2, ...)"""
    i = np.arange(-pad, n + pad)
    i = np.where(i < 0, -i, i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def _min_eigen_f64(image):
    """cornerMinEigenVal(blockSize 3, ksize 3) in float64, written apart from sr.min_eigen: integer Sobel on the reflect-101
    padded image, products in float64, unnormalised 3x3 box sums of the reflect-101 padded products, closed-form smaller
    eigenvalue of [[Sxx, Sxy], [Sxy, Syy]] / 2.  -> (eig, (Sxx + Syy) / 2), both [rows, cols] float64"""
    img = np.asarray(image, np.int64)
    rows, cols = img.shape
    p = img[_reflect101_index(rows, 1)][:, _reflect101_index(cols, 1)]
    sx = np.zeros((rows, cols), np.int64)
    sy = np.zeros((rows, cols), np.int64)
    for k, w in ((0, 1), (1, 2), (2, 1)):
        sx += w * (p[k:k + rows, 2:] - p[k:k + rows, :-2])
        sy += w * (p[2:, k:k + cols] - p[:-2, k:k + cols])
    dx, dy = sx / 3060.0, sy / 3060.0  # 4 * 3 * 255
    ri, ci = _reflect101_index(rows, 1), _reflect101_index(cols, 1)
    box = []
    for q in (dx * dx, dx * dy, dy * dy):
        qp = q[ri][:, ci]
        box.append(sum(qp[a:a + rows, b:b + cols] for a in range(3) for b in range(3)))
    sxx, sxy, syy = box
    half = (sxx + syy) / 2
    return half - np.sqrt(((sxx - syy) / 2) ** 2 + sxy ** 2), half


# |eig32 - eig64| <= C * 2^-24 * (Sxx + Syy) / 2, with u = 2^-24 and T = (Sxx + Syy) / 2 = a + c (a = Sxx / 2, c = Syy / 2, b = Sxy):
#   dx = fl(sx * fl(1/3060)): 2u relative (the integer Sobel converts exactly); a product dx * dy: 2u + 2u + u = 5u relative;
#   a box sum passes every product through four additions: Sxx, Syy within 9u relative, Sxy within 9u * sum |dx dy| <= 9u * T
#   (|dx dy| <= (dx^2 + dy^2) / 2).  So |da| + |dc| <= 9u T and |db| <= 9u T.
#   R = sqrt((a - c)^2 + b^2) <= T (Cauchy-Schwarz: b^2 <= 4ac) is 1-Lipschitz in (a - c, b): the inputs move it by <= 18u T.
#   The formula's own roundings: a + c (u T), a - c (u T through R), d*d + b*b and the square root (2u R <= 2u T), the final
#   subtraction (u |eig| <= u T).  Together 9 + 18 + 1 + 1 + 2 + 1 = 32 u T to first order; C = 33 covers the second-order terms
#   (below 1e3 u^2 T) and the float64 reference's own rounding (below 1e2 * 2^-53 T).
# The error scales with T, not with |eig|: the cancellation in (a + c) - R loses what a and c carry of T.
C_EIG = 33


def _bound_images():
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[:96, :128]
    blocky = np.repeat(np.repeat(rng.integers(0, 256, (16, 22)), 6, 0), 6, 1)[:96, :128]
    return {
        "kitti": rp.kitti_image("left", 0),
        "icl": rp.icl_gray(0),
        "random": rng.integers(0, 256, (120, 200)),
        "blocky": blocky,
        "ramp": (3 * xx + 6 * yy) % 256,
        "ramp_x2y": (xx + 2 * yy) % 256,
        "stripes": np.sin((xx + 2 * yy) * 0.3) * 100 + 128,
    }


@pytest.mark.parametrize("name", list(_bound_images()))
def test_min_eigen_within_the_float32_bound_of_a_float64_evaluation(name):
    img = np.asarray(_bound_images()[name]).astype(np.uint8)
    e32 = sr.min_eigen(img).astype(np.float64)
    e64, half = _min_eigen_f64(img)
    assert (half >= 0).all() and (e64 >= -1e-12 * np.maximum(half, 1e-30)).all()  # positive semidefinite up to float64 rounding
    err = np.abs(e32 - e64)
    bound = C_EIG * 2.0 ** -24 * half
    assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
    # the float32 arithmetic really is what is measured: somewhere the difference is not zero
    assert err.max() > 0
