"""Both feature extractors at their shape, pitch and capacity edges, each case against its checker: the C oracle
(oracle.binding_features.extract_features) for FAST + ORB, tests/selective_ref.py for the selective GFTT extractor.  Keypoints
in order, intensities and descriptors byte for byte, n_features and status.  Where a case exists to reach a path, it also
asserts from the checker or from the host formula restated below that the path is reached (tile variants, raw detection
counts, candidate counts, cell doubling, chunk conflicts), so an edge cannot drift away from its case unnoticed."""
import numpy as np
import pytest
import torch

import ref_pins as rp
import selective_ref as sr
from helpers import corr_equal
from oracle import binding_features as of
from srrg2_proslam_amd import ops

pytestmark = pytest.mark.gpu

OK, WARN_NO_MATCHES, ERR_CAPACITY, ERR_RANGE, ERR_UNSUPPORTED = 0, 2, -2, -4, -5
DEV = torch.device("cuda", 0)
NO_PROJ = np.zeros((0, 2), np.float32)


# ---- images -------------------------------------------------------------------------------------------------------------
def smooth_noise(rng, rows, cols, f=3):
    """bilinear upsampling of random values by f: corners everywhere, no ties between neighbouring FAST responses"""
    g = rng.integers(0, 256, (rows // f + 2, cols // f + 2)).astype(np.float32)
    yi, xi = np.arange(rows) / f, np.arange(cols) / f
    y0, x0 = yi.astype(int), xi.astype(int)
    fy, fx = (yi - y0)[:, None], (xi - x0)[None, :]
    top = g[y0][:, x0] * (1 - fx) + g[y0][:, x0 + 1] * fx
    bot = g[y0 + 1][:, x0] * (1 - fx) + g[y0 + 1][:, x0 + 1] * fx
    return (top * (1 - fy) + bot * fy).astype(np.uint8)


def kitti_crop(i, rows, cols, y=0, x=0):
    k = rp.kitti_image("left", i)
    return np.ascontiguousarray(k[y:y + rows, x:x + cols])


def kitti_mosaic(rows, cols):
    """KITTI frames tiled (alternately mirrored) over a large canvas"""
    frames = [rp.kitti_image("left", i) for i in range(3)]
    out = np.zeros((rows, cols), np.uint8)
    for y in range(0, rows, 376):
        for x in range(0, cols, 1241):
            t = frames[(y // 376 + x // 1241) % 3]
            t = t[::-1] if (y // 376) % 2 else t
            t = t[:, ::-1] if (x // 1241) % 2 else t
            out[y:y + 376, x:x + 1241] = t[:min(376, rows - y), :min(1241, cols - x)]
    return out


def dots(rows, cols, positions, values, background=30):
    """isolated single bright pixels: each one is exactly one FAST detection and one GFTT candidate"""
    img = np.full((rows, cols), background, np.uint8)
    for (y, x), v in zip(positions, values):
        img[y, x] = v
    return img


def lattice(lo_y, hi_y, lo_x, hi_x, step=8):
    return [(y, x) for y in range(lo_y, hi_y, step) for x in range(lo_x, hi_x, step)]


# ---- FAST: device runs and checks -----------------------------------------------------------------------------------------
def fast_raw_count(img, threshold):
    """post-suppression detections of an image (what max_raw_detections bounds): score > 0 and above all eight neighbours"""
    s = of.fast_scores(img, threshold).astype(np.int32)
    p = np.pad(s, 1)
    m = np.zeros_like(s)
    for dy in range(3):
        for dx in range(3):
            if dy != 1 or dx != 1:
                m = np.maximum(m, p[dy:dy + s.shape[0], dx:dx + s.shape[1]])
    return int(((s > 0) & (s > m)).sum())


def device_images(images, pad=0, seed=0):
    """[B, rows, cols] uint8 on the device; pad > 0: a view into a buffer whose rows are pad bytes longer (pitch = cols + pad),
    the padding filled with noise so that any read of it changes a result"""
    host = np.stack(images)
    if not pad:
        return torch.from_numpy(host).to(DEV).contiguous()
    B, rows, cols = host.shape
    big = np.random.default_rng(seed).integers(0, 256, (B, rows, cols + pad), dtype=np.uint8)
    big[:, :, :cols] = host
    view = torch.from_numpy(big).to(DEV)[:, :, :cols]
    assert view.stride(1) == cols + pad and not view.is_contiguous()
    return view


def run_fast(ctx, pg, images, stride, pad=0):
    B = len(images)
    img = device_images(images, pad)
    kp = torch.zeros((B, stride, 2), dtype=torch.float32, device=DEV)
    desc = torch.zeros((B, stride, 32), dtype=torch.uint8, device=DEV)
    inten = torch.zeros((B, stride), dtype=torch.float32, device=DEV)
    n = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    st = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ops.extract_features_batch(ctx, pg, img, kp, desc, n, st, inten)
    ctx.synchronize()
    return kp.cpu().numpy(), desc.cpu().numpy(), inten.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()


def fast_params(threshold=15, nms=1, target=1000, grid=(3, 3), std=False, max_raw=32768):
    po = of.extractor_params(threshold, nms, target, grid[0], grid[1], of.SELECT_LIBSTDCXX if std else of.SELECT_CANONICAL)
    pg = ops.extractor_params(threshold, nms, target, grid[0], grid[1], ops.SELECT_LIBSTDCXX if std else ops.SELECT_CANONICAL, max_raw)
    return po, pg


def check_fast(po, images, out, expect=None):
    """every image equals the oracle; expect[b] < 0: that image fails with exactly that status and no features"""
    kp, desc, inten, n, st = out
    refs = []
    for b, img in enumerate(images):
        if expect is not None and expect[b] < 0:
            assert st[b] == expect[b] and n[b] == 0, (b, st[b], n[b])
            refs.append(None)
            continue
        uv, oi, od = of.extract_features(po, img, capacity=max(kp.shape[1], 1) + 1)
        k = len(uv)
        assert st[b] == (OK if k else WARN_NO_MATCHES) and n[b] == k, (b, st[b], n[b], k)
        assert np.array_equal(kp[b, :k], uv), b
        assert np.array_equal(inten[b, :k], oi), b
        assert np.array_equal(desc[b, :k], od), b
        refs.append(uv)
    return refs


def tiles(rows, cols, w=64, h=64):
    """the host's tile grid and, per tile, whether fast_blur_kernel / blur_kernel take the interior instantiation"""
    return {(x0, y0): x0 >= 4 and x0 + w + 4 <= cols and y0 >= 4 and y0 + h + 4 <= rows
            for y0 in range(0, rows, h) for x0 in range(0, cols, w)}


def raises(status, fn, *args, **kw):
    with pytest.raises(ops.ProslamHipError) as e:
        fn(*args, **kw)
    assert e.value.status == status, e.value.status


# ---- FAST: shapes ---------------------------------------------------------------------------------------------------------
EDGES = (127, 128, 129, 131, 132, 133, 195, 196, 197)
# interior tile columns (x0) per side length: x0 = 64 from 132 on, x0 = 128 from 196 on
INTERIOR = {127: [], 128: [], 129: [], 131: [], 132: [64], 133: [64], 195: [64], 196: [64, 128], 197: [64, 128]}
SHAPES = [(s, 200) for s in EDGES] + [(200, s) for s in EDGES] + [(200, 143), (200, 145), (120, 207), (120, 209), (62, 200), (200, 62), (63, 97)]


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_fast_shapes_around_tiles_and_the_interior_switch(hip_ctx, rows, cols):
    images = [smooth_noise(np.random.default_rng(rows * 1000 + cols), rows, cols), kitti_crop(rows % 3, rows, cols, 100, 300)]
    po, pg = fast_params(15, 1, 10 ** 5, (2, 3))
    refs = check_fast(po, images, run_fast(hip_ctx, pg, images, 4096))
    t = tiles(rows, cols)
    assert len(t) == ((rows + 63) // 64) * ((cols + 63) // 64)
    if rows == 200 and cols in INTERIOR:  # the side under test is the width
        assert sorted({x0 for (x0, y0), inner in t.items() if inner}) == INTERIOR[cols]
    if cols == 200 and rows in INTERIOR:
        assert sorted({y0 for (x0, y0), inner in t.items() if inner}) == INTERIOR[rows]
    if min(rows, cols) < 63:
        assert all(len(r) == 0 for r in refs)  # the ORB border leaves nothing: the case only runs the code
        return
    uv = refs[0]
    assert len(uv) > 0
    for seam in (64, 128, 192):  # the texture puts keypoints next to every tile seam that lies inside the ORB border
        if 34 <= seam <= cols - 35:
            assert np.any(np.abs(uv[:, 0] - seam + 0.5) <= 2.5), ("column seam", seam)
        if 34 <= seam <= rows - 35:
            assert np.any(np.abs(uv[:, 1] - seam + 0.5) <= 2.5), ("row seam", seam)


def test_fast_wide_and_tall_images(hip_ctx):
    po, pg = fast_params(15, 1, 3000, (2, 8), max_raw=32768)
    for rows, cols in ((96, 8192), (8192, 96)):
        img = smooth_noise(np.random.default_rng(rows), rows, cols, 5)
        assert fast_raw_count(img, 15) <= 32768
        refs = check_fast(po, [img], run_fast(hip_ctx, pg, [img], 4096))
        assert len(refs[0]) > 500


def test_fast_largest_image_and_the_first_refused(hip_ctx):
    """4096 x 4095 = 2^24 - 4096 pixels is the largest accepted image (pixel indices share a word with the 8-bit response);
    4096 x 4096 is refused"""
    img = kitti_mosaic(4096, 4095)
    po, pg = fast_params(80, 1, 4000, (4, 4), max_raw=32768)
    uv = check_fast(po, [img], run_fast(hip_ctx, pg, [img], 8192))[0]
    assert len(uv) > 2000 and uv[:, 0].max() >= 4032 and uv[:, 1].max() >= 4032  # keypoints in the last tile row and column
    big = torch.zeros((1, 4096, 4096), dtype=torch.uint8, device=DEV)
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
    raises(ERR_UNSUPPORTED, ops.extract_features_batch, hip_ctx, pg, big, z(1, 16, 2), z(1, 16, 32, dt=torch.uint8), z(1, dt=torch.int32), z(1, dt=torch.int32))


def test_fast_smallest_images(hip_ctx):
    po, pg = fast_params(10, 1, 100, (1, 1))
    rng = np.random.default_rng(4)
    images = [rng.integers(0, 256, (7, 7), dtype=np.uint8) for _ in range(2)]
    out = run_fast(hip_ctx, pg, images, 16)
    check_fast(po, images, out)
    assert (out[4] == WARN_NO_MATCHES).all() and (out[3] == 0).all()  # accepted, nothing inside the ORB border
    for rows, cols in ((6, 7), (7, 6)):
        img = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
        raises(ERR_UNSUPPORTED, ops.extract_features, hip_ctx, pg, img)


# ---- FAST: pitch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(200, 264), (131, 197)])
def test_fast_pitch_wider_than_the_image(hip_ctx, rows, cols):
    rng = np.random.default_rng(cols)
    images = [smooth_noise(rng, rows, cols), kitti_crop(1, rows, cols, 50, 500), smooth_noise(rng, rows, cols, 5)]
    po, pg = fast_params(12, 1, 1500, (3, 3), std=True)
    base = run_fast(hip_ctx, pg, images, 4096)
    check_fast(po, images, base)
    assert base[3].min() > 100
    for pad in (13, 64):
        got = run_fast(hip_ctx, pg, images, 4096, pad=pad)
        for a, b in zip(base, got):
            assert np.array_equal(a, b), pad


# ---- FAST: raw detection capacity ---------------------------------------------------------------------------------------------
def dot_image(count, rows=280, cols=280, seed=0):
    pos = lattice(8, rows - 8, 8, cols - 8)
    assert len(pos) >= count
    vals = np.random.default_rng(seed).integers(120, 256, count)
    return dots(rows, cols, pos[:count], vals)


@pytest.mark.parametrize("nms", [1, 0])
def test_fast_raw_detection_capacity_edges(hip_ctx, nms):
    """max_raw_detections is rounded up to a power of two of at least 1024: 1024 dots fit 1024, 1025 fail only their image,
    and 1025 fit when 1025 is asked for (2048)"""
    images = [dot_image(1024, seed=1), dot_image(1025, seed=2), dot_image(1024, seed=3)]
    for img, k in zip(images, (1024, 1025, 1024)):
        assert (of.fast_scores(img, 15) != 0).sum() == k and fast_raw_count(img, 15) == k
    po, _ = fast_params(15, nms, 10 ** 6, (1, 1))
    for max_raw, expect in ((1024, [OK, ERR_CAPACITY, OK]), (1025, None), (0, None)):
        _, pg = fast_params(15, nms, 10 ** 6, (1, 1), max_raw=max_raw)
        check_fast(po, images, run_fast(hip_ctx, pg, images, 1100), expect)


def test_fast_raw_detection_limit(hip_ctx):
    """32768 raw detections fill the selection's LDS keys and its 15-bit detection index; 32769 fail; max_raw 32769 is refused"""
    pos = lattice(8, 1464, 8, 1464)
    images = [dots(1472, 1472, pos[:k], np.full(k, 200)) for k in (32768, 32769)]
    assert [fast_raw_count(img, 15) for img in images] == [32768, 32769]
    po, pg = fast_params(15, 1, 10 ** 6, (1, 1), max_raw=32768)
    check_fast(po, images, run_fast(hip_ctx, pg, images, 32768), [OK, ERR_CAPACITY])
    raises(ERR_UNSUPPORTED, ops.extract_features, hip_ctx, ops.extractor_params(max_raw_detections=32769), images[0])


# ---- FAST: regions and thresholds -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("std", [False, True])
@pytest.mark.parametrize("grid,target", [((16, 16), 3000), ((1, 16), 1000), ((16, 1), 1000), ((16, 16), 100), ((4, 4), 10)])
def test_fast_regions(hip_ctx, std, grid, target):
    images = [rp.kitti_image("left", 0), rp.kitti_image("right", 2)]
    po, pg = fast_params(15, 1, target, grid, std)
    refs = check_fast(po, images, run_fast(hip_ctx, pg, images, 4096))
    if target < grid[0] * grid[1]:  # target_per = 0: no region keeps anything
        assert all(len(r) == 0 for r in refs)
    else:
        assert all(len(r) > 0 for r in refs)


def test_fast_region_limit(hip_ctx):
    img = rp.kitti_image("left", 0)
    raises(ERR_UNSUPPORTED, ops.extract_features, hip_ctx, ops.extractor_params(vertical=1, horizontal=257), img)
    raises(ERR_UNSUPPORTED, ops.extract_features, hip_ctx, ops.extractor_params(threshold=0), img)
    raises(ERR_UNSUPPORTED, ops.extract_features, hip_ctx, ops.extractor_params(threshold=255), img)


@pytest.mark.parametrize("std", [False, True])
def test_fast_extreme_thresholds(hip_ctx, std):
    rng = np.random.default_rng(8)
    # threshold 1: every slope is a corner candidate
    images = [smooth_noise(rng, 200, 264, 5), kitti_crop(0, 200, 264, 100, 600)]
    po, pg = fast_params(1, 1, 1000, (2, 2), std)
    refs = check_fast(po, images, run_fast(hip_ctx, pg, images, 4096))
    assert all(len(r) > 200 for r in refs)
    # threshold 254: a 255 dot on black is a corner (255 > 0 + 254), a 254 dot is not
    pos = lattice(40, 160, 40, 224)
    vals = np.where(np.arange(len(pos)) % 3 == 0, 254, 255)
    img = dots(200, 264, pos, vals, background=0)
    po, pg = fast_params(254, 1, 1000, (2, 2), std)
    uv = check_fast(po, [img], run_fast(hip_ctx, pg, [img], 1024))[0]
    assert len(uv) == int((vals == 255).sum())


# ---- FAST: describe_kernel's folding of image and 96-keypoint chunk ------------------------------------------------------------
COUNTS = (95, 96, 97, 191, 192, 193, 1, 0)


def counted_images(B, seed):
    """dot images with exactly COUNTS[b % 8] keypoints, all inside the ORB border, distinct positions and intensities"""
    rng = np.random.default_rng(seed)
    pos = lattice(32, 192, 32, 192)  # 20 x 20 sites inside [31, 224 - 31)
    out = []
    for b in range(B):
        k = COUNTS[b % len(COUNTS)]
        pick = rng.choice(len(pos), k, replace=False)
        out.append(dots(224, 224, [pos[i] for i in pick], rng.integers(100, 256, k)))
    return out


@pytest.mark.parametrize("B", [7, 8, 9, 17])
def test_describe_folding_across_images_and_chunks(hip_ctx, B):
    images = counted_images(B, B)
    po, pg = fast_params(15, 1, 10 ** 6, (1, 1))
    counts = [COUNTS[b % len(COUNTS)] for b in range(B)]
    for img, k in zip(images, counts):
        assert len(of.extract_features(po, img)[0]) == k
    for stride in (193, 192, 97, 96):
        expect = [ERR_CAPACITY if k > stride else OK for k in counts]
        check_fast(po, images, run_fast(hip_ctx, pg, images, stride), expect)


# ---- selective: device runs and checks -----------------------------------------------------------------------------------------
def run_sel(ctx, p, images, projections=None, radius=None, stride=4096, masks=None, pad=0, n_projections=None, projection_stride=None):
    B = len(images)
    img = device_images(images, pad, seed=1)
    kp = torch.zeros((B, stride, 2), dtype=torch.float32, device=DEV)
    desc = torch.zeros((B, stride, 32), dtype=torch.uint8, device=DEV)
    inten = torch.zeros((B, stride), dtype=torch.float32, device=DEV)
    n = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    st = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    kw = {}
    if projections is not None:
        P = projection_stride or max(1, max(len(q) for q in projections))
        proj = np.zeros((B, P, 2), np.float32)
        for b, q in enumerate(projections):
            proj[b, :len(q)] = q
        counts = n_projections if n_projections is not None else [len(q) for q in projections]
        kw = dict(projections=torch.from_numpy(proj).to(DEV), n_projections=torch.tensor(counts, dtype=torch.int32, device=DEV))
    if radius is not None:
        kw["radius"] = torch.tensor(radius, dtype=torch.int32, device=DEV)
    if masks is not None:
        kw["seeding_mask"] = device_images(masks, pad, seed=2)
    ops.extract_features_selective_batch(ctx, p, img, kp, desc, n, st, inten, **kw)
    ctx.synchronize()
    return kp.cpu().numpy(), desc.cpu().numpy(), inten.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()


def check_sel(out, refs, expect=None):
    """refs[b] = sr.extract(...) of image b; expect[b] < 0: the image fails with that status and no features"""
    kp, desc, inten, n, st = out
    for b, ref in enumerate(refs):
        if expect is not None and expect[b] < 0:
            assert st[b] == expect[b] and n[b] == 0, (b, st[b], n[b])
            continue
        k = len(ref[0])
        assert st[b] == (OK if k else WARN_NO_MATCHES) and n[b] == k, (b, st[b], n[b], k)
        assert np.array_equal(kp[b, :k], ref[0]), b
        assert np.array_equal(inten[b, :k], ref[1]), b
        assert np.array_equal(desc[b, :k], ref[2]), b


def sel_params(target=1000, width=10, max_candidates=0, descriptor="ORB-256", seeding=True, left=False, right=False):
    return ops.selective_extractor_params("GFTT", descriptor, target, width, left, right, seeding, max_candidates=max_candidates)


def grid_doublings(rows, cols, md, max_candidates=0):
    """selective_extract_launch's minimum-distance grid: cells of md, doubled while there are more cells than sort_n"""
    cap = max_candidates or 8192
    sort_n = 2
    while sort_n < cap:
        sort_n *= 2
    cell, k = max(md, 1), 0
    while md > 0 and -(-cols // cell) * -(-rows // cell) > sort_n:
        cell, k = cell * 2, k + 1
    return k, cell


def projections(rng, rows, cols, count):
    return np.stack([rng.uniform(0, cols - 0.5, count), rng.uniform(0, rows - 0.5, count)], 1).astype(np.float32)


# ---- selective: shapes ------------------------------------------------------------------------------------------------------------
SEL_SHAPES = [(8, 8), (79, 200), (80, 200), (81, 200), (120, 127), (120, 128), (120, 129), (80, 4096), (4096, 80)]


@pytest.mark.parametrize("tracking", [False, True])
@pytest.mark.parametrize("rows,cols", SEL_SHAPES)
def test_selective_shapes(hip_ctx, rows, cols, tracking):
    rng = np.random.default_rng(rows + 7 * cols)
    images = [smooth_noise(rng, rows, cols, 4), smooth_noise(rng, rows, cols, 9)]
    proj = [projections(rng, rows, cols, 40), NO_PROJ] if tracking else None
    radius = [3, 0] if tracking else None
    p = sel_params(800, 6, max_candidates=16384)
    refs = [sr.extract(img, 800, 6, projections=None if proj is None else proj[b], radius=0 if radius is None else radius[b])
            for b, img in enumerate(images)]
    for img in images:
        assert len(sr.candidates(img, None)[0]) <= 16384
    check_sel(run_sel(hip_ctx, p, images, proj, radius, stride=2048), refs)
    assert ((cols + 31) // 32 == 128) == (cols == 4096)  # 80 x 4096: mask_raster_kernel's 128 words per row, LDS of 8 x 4097 ints
    if (rows, cols) == (8, 8):
        assert all(len(r[0]) == 0 for r in refs)
    elif min(rows, cols) >= 79:
        assert len(refs[0][0]) > 0


def test_selective_refused_sides(hip_ctx):
    p = sel_params()
    for rows, cols in ((7, 8), (8, 7), (4097, 80), (80, 4097)):
        img = np.zeros((rows, cols), np.uint8)
        raises(ERR_UNSUPPORTED, ops.extract_features_selective, hip_ctx, p, img)


# ---- selective: pitch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [13, 64])
def test_selective_pitch_wider_than_the_image(hip_ctx, pad):
    rng = np.random.default_rng(pad)
    rows, cols = 131, 197
    images = [smooth_noise(rng, rows, cols, 4), kitti_crop(2, rows, cols, 80, 400), smooth_noise(rng, rows, cols, 7)]
    masks = [(rng.uniform(size=(rows, cols)) < 0.6).astype(np.uint8) for _ in images]
    p = sel_params(400, 5)
    # seeding with an external mask (mask_raster_kernel reads it at the images' pitch)
    refs = [sr.extract(img, 400, 5, external_mask=m) for img, m in zip(images, masks)]
    base = run_sel(hip_ctx, p, images, masks=masks)
    check_sel(base, refs)
    got = run_sel(hip_ctx, p, images, masks=masks, pad=pad)
    assert all(np.array_equal(a, b) for a, b in zip(base, got))
    # tracking plus seeding
    proj = [projections(rng, rows, cols, 25) for _ in images]
    refs = [sr.extract(img, 400, 5, projections=q, radius=4) for img, q in zip(images, proj)]
    base = run_sel(hip_ctx, p, images, proj, [4, 4, 4])
    check_sel(base, refs)
    got = run_sel(hip_ctx, p, images, proj, [4, 4, 4], pad=pad)
    assert all(np.array_equal(a, b) for a, b in zip(base, got))


# ---- selective: minimum distance grid -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descriptor", ["ORB-256", "BRIEF-256"])
def test_selective_min_distance_grid(hip_ctx, descriptor):
    img = rp.kitti_image("left", 0)
    rows, cols = img.shape
    eig = sr.min_eigen(img)
    widths = (0, 1, 4, 7, 8, 4096)
    # with 8192 candidates (sort_n 8192) the cells double for widths 1 .. 7 on KITTI, not from 8 on; 4096 is one cell
    assert [grid_doublings(rows, cols, w)[0] for w in widths] == [0, 3, 1, 1, 0, 0]
    assert grid_doublings(rows, cols, 4096)[1] == 4096
    images, refs = [], []
    for w in widths:
        ref = sr.extract(img, 1000, w, eig=eig)
        kp, desc, inten, n, st = run_sel(hip_ctx, sel_params(1000, w, descriptor=descriptor), [img])
        check_sel((kp, desc, inten, n, st), [ref])
        refs.append(len(ref[0]))
    assert refs[-1] == 1 and min(refs) > 0
    # sort_n 1024: two doublings of 10-px cells; a seeding mask keeps the candidates below max_candidates = 1000
    mask = np.zeros_like(img)
    mask[:, 200:360] = 1
    assert len(sr.candidates(img, mask, eig)[0]) < 1000 < len(sr.candidates(img, None, eig)[0])
    assert grid_doublings(rows, cols, 10, 1000) == (2, 40)
    ref = sr.extract(img, 1000, 10, external_mask=mask, eig=eig)
    check_sel(run_sel(hip_ctx, sel_params(1000, 10, 1000, descriptor), [img], masks=[mask]), [ref])
    assert len(ref[0]) > 100


# ---- selective: the 64-candidate chunks of the greedy pass --------------------------------------------------------------------------
def chunk_image(count, seed):
    """dots with exactly `count` GFTT candidates: singles on a 16-px lattice and pairs 5 px apart (closer than minDistance 8)"""
    rng = np.random.default_rng(seed)
    sites = lattice(40, 168, 40, 328, 16)
    n_pairs = count // 3
    n_sites = count - n_pairs
    pick = rng.choice(len(sites), n_sites, replace=False)
    pos = [sites[i] for i in pick]
    pos += [(y, x + 5) for (y, x) in pos[:n_pairs]]
    return dots(208, 368, pos, rng.integers(120, 256, len(pos)), background=20)


def greedy_trace(ys, xs, md, maxc):
    """the greedy min-distance pass over the sorted candidates: accepted indices and (rejected, conflicting accepted) pairs"""
    acc, rej = [], []
    for i, (y, x) in enumerate(zip(ys.tolist(), xs.tolist())):
        hit = next((j for j in acc if (xs[j] - x) ** 2 + (ys[j] - y) ** 2 < md * md), None)
        if hit is None:
            acc.append(i)
            if len(acc) == maxc:
                break
        else:
            rej.append((i, hit))
    return acc, rej


@pytest.mark.parametrize("count", [1, 63, 64, 65, 127, 128, 129])
def test_selective_greedy_chunks(hip_ctx, count):
    img = chunk_image(count, {65: 60}.get(count, count))  # (seed 60: the 65th candidate is rejected by the first chunk)
    ys, xs = sr.candidates(img, None)
    assert len(ys) == count
    acc, rej = greedy_trace(ys, xs, 8, 1000)
    assert np.array_equal(np.stack([xs[acc], ys[acc]], 1), sr.gftt(img, None, 1000, 8))
    if count > 64:  # some rejections conflict with a candidate of an earlier chunk, some with one of the same chunk
        assert any(j // 64 < i // 64 for i, j in rej) and any(j // 64 == i // 64 for i, j in rej)
    elif count > 1:
        assert rej
    cases = [(1000, None)]
    if count > 120:  # maxCorners reached in the middle of the second chunk
        target = len([i for i in acc if i < 64 + 20])
        cases.append((target, acc[target - 1]))
    for target, last in cases:
        if last is not None:
            assert last % 64 not in (0, 63) and last // 64 == 1 and last < count - 1
        ref = sr.extract(img, target, 8)
        assert len(ref[0]) == min(target, len(acc))
        check_sel(run_sel(hip_ctx, sel_params(target, 8), [img]), [ref])


# ---- selective: LDS and candidate edges ----------------------------------------------------------------------------------------------
def test_selective_lds_and_candidate_edges(hip_ctx):
    img = rp.kitti_image("left", 0)
    eig = sr.min_eigen(img)
    # sort_n * 8 + maxCorners * 8 == 160 KiB exactly: runs; one more keypoint: refused
    assert 16384 * 8 + 4096 * 8 == 160 * 1024
    ref = sr.extract(img, 4096, 1, eig=eig)
    check_sel(run_sel(hip_ctx, sel_params(4096, 1, 16384), [img]), [ref])
    raises(ERR_UNSUPPORTED, ops.extract_features_selective, hip_ctx, sel_params(4097, 1, 16384), img)
    raises(ERR_UNSUPPORTED, ops.extract_features_selective, hip_ctx, sel_params(1000, 10, 16385), img)
    # max_candidates that is not a power of two (sort_n 8192)
    assert len(sr.candidates(img, None, eig)[0]) < 5000
    ref = sr.extract(img, 1500, 3, eig=eig)
    check_sel(run_sel(hip_ctx, sel_params(1500, 3, 5000), [img]), [ref])


def test_selective_capacity_with_both_runs(hip_ctx):
    img = rp.kitti_image("left", 1)
    eig = sr.min_eigen(img)
    rows, cols = img.shape
    proj = projections(np.random.default_rng(3), rows, cols, 60)
    t = sr.tracking_mask(rows, cols, proj, 5)
    n0 = len(sr.describe(img, sr.gftt(img, t, 500, 10, eig=eig))[0])
    n1 = len(sr.describe(img, sr.gftt(img, 1 - t, 500, 10, eig=eig))[0])
    assert n0 > 0 and n1 > 0
    ref = sr.extract(img, 500, 10, projections=proj, radius=5, eig=eig)
    assert len(ref[0]) == n0 + n1
    flat = np.full_like(img, 90)
    p = sel_params(500, 10)
    for stride, status in ((n0 + n1, OK), (n0 + n1 - 1, ERR_CAPACITY)):
        out = run_sel(hip_ctx, p, [img, flat], [proj, proj], [5, 5], stride=stride)
        check_sel(out, [ref, sr.extract(flat, 500, 10, projections=proj, radius=5)], [status, OK])


# ---- selective: per-image range errors ---------------------------------------------------------------------------------------------
def test_selective_range_errors_leave_the_batch_exact(hip_ctx):
    rng = np.random.default_rng(12)
    rows, cols = 120, 200
    P = 8
    good = lambda: projections(rng, rows, cols, 6)
    with_bad = lambda uv: np.concatenate([good(), np.array([uv], np.float32)])
    cases = [  # (projections, n_projections or None, radius, expected)
        (NO_PROJ, None, 0, OK),
        (with_bad((np.nan, 10.0)), None, 2, ERR_RANGE),
        (with_bad((10.0, np.nan)), None, 2, ERR_RANGE),
        (with_bad((-0.25, 10.0)), None, 2, ERR_RANGE),
        (with_bad((10.0, -1.0)), None, 2, ERR_RANGE),
        (with_bad((10.0, float(rows))), None, 2, ERR_RANGE),
        (with_bad((float(cols), 10.0)), None, 2, ERR_RANGE),
        (good(), None, -1, ERR_RANGE),
        (good(), None, 4097, ERR_RANGE),
        (good(), -1, 0, ERR_RANGE),
        (good(), P + 1, 0, ERR_RANGE),
        # valid edges: u = 0, u = cols - 0.5 and v = rows - 0.5 (both round to one past the image), the largest radius
        (np.array([(0.0, 50.0), (cols - 0.5, rows - 0.5), (cols - 0.5, 0.0), (0.0, rows - 0.5)], np.float32), None, 3, OK),
        (good(), None, 4096, OK),
        (good(), P, 1, OK),
    ]
    images = [smooth_noise(rng, rows, cols, 4) for _ in cases]
    proj = [c[0] for c in cases]
    counts = [len(c[0]) if c[1] is None else c[1] for c in cases]
    expect = [c[3] for c in cases]
    pad = [np.concatenate([q, projections(rng, rows, cols, P - len(q))]) if len(q) < P else q for q in proj]
    p = sel_params(300, 5)
    out = run_sel(hip_ctx, p, images, pad, [c[2] for c in cases], n_projections=counts, projection_stride=P)
    refs = []
    for b, img in enumerate(images):
        refs.append(None if expect[b] < 0 else sr.extract(img, 300, 5, projections=pad[b][:counts[b]], radius=cases[b][2]))
    check_sel(out, refs, expect)
    # the half-pixel projections really reach one past the image
    assert sr.round_half_away(np.float32(cols - 0.5)) == cols and sr.round_half_away(np.float32(rows - 0.5)) == rows


# ---- selective: responses made of rounding --------------------------------------------------------------------------------------------
def test_selective_rounding_dominated_responses(hip_ctx):
    rows, cols = 96, 128
    yy, xx = np.mgrid[:rows, :cols]
    images, masks, kinds = [], [], []
    # (3x + 6y) mod 256 and (x + 16y) mod 256: inside each band the gradient is constant and the structure tensor singular, so
    # the response is float32 rounding of an exact zero (+1.2e-10, +9.3e-10); the seeding mask keeps the 5x5 windows off the
    # wrap lines, so the maximum, the threshold and every candidate are rounding noise
    for a, b, lo in ((3, 6, 20), (1, 16, 36)):
        lin = a * xx + b * yy
        images.append((lin % 256).astype(np.uint8))
        m = ((lin % 256 >= lo) & (lin % 256 < 256 - lo)).astype(np.uint8)
        m[:3], m[-3:], m[:, :3], m[:, -3:] = 0, 0, 0, 0  # (and off the reflected border)
        masks.append(m)
        kinds.append("noise")
    # x + 2y without a mask: a negative rounding response (-1.5e-11) inside, real corners only where the reflected border bends it
    images.append(((xx + 2 * yy) % 256).astype(np.uint8))
    masks.append(np.ones((rows, cols), np.uint8))
    kinds.append("ramp")
    # stripes along 45 degrees: the exact zero of the interior (dx == dy) against the structure the reflected border adds
    images.append((np.sin((xx + yy) * 0.5) * 100 + 128).astype(np.uint8))
    masks.append(np.ones((rows, cols), np.uint8))
    kinds.append("diagonal")
    # vertical and horizontal stripes and a constant image: every response is exactly 0, there is no candidate
    images += [(np.sin(xx * 0.7) * 100 + 128).astype(np.uint8), (np.sin(yy * 0.9) * 100 + 128).astype(np.uint8), np.full((rows, cols), 77, np.uint8)]
    masks += [np.ones((rows, cols), np.uint8)] * 3
    kinds += ["zero"] * 3
    for img, m, kind in zip(images, masks, kinds):
        e = sr.min_eigen(img)
        if kind == "noise":
            ys, xs = sr.candidates(img, m, e)
            vals = np.unique(e[ys, xs])
            assert len(ys) > 1000 and len(vals) == 1 and 0 < vals[0] < 1e-9, (len(ys), vals)
        elif kind == "ramp":
            assert (e[2:-2, 2:50] < 0).all()  # (left of the first wrap line)
        elif kind == "diagonal":
            assert not e[2:-2, 2:-2].any() and e.any()
        else:
            assert not e.any()
    p = sel_params(1000, 6, 16384)
    refs = [sr.extract(img, 1000, 6, external_mask=m) for img, m in zip(images, masks)]
    assert all(len(r[0]) > 0 for r, k in zip(refs, kinds) if k == "noise")
    check_sel(run_sel(hip_ctx, p, images, masks=masks), refs)


# ---- one context, both extractors, scratch slots growing and shrinking -----------------------------------------------------------------
def test_one_context_both_extractors(oracle):
    ctx = ops.Context(0)
    try:
        kitti = [rp.kitti_image("left", 0), rp.kitti_image("right", 0), rp.kitti_image("left", 2)]
        po, pg = fast_params(15, 1, 1000, (3, 3))
        first = run_fast(ctx, pg, kitti, 2048)
        check_fast(po, kitti, first)

        icl = [rp.icl_gray(k) for k in (0, 1, 50)] + [rp.icl_gray(0)[::-1].copy(), rp.icl_gray(1)[:, ::-1].copy()]
        rng = np.random.default_rng(21)
        proj = [projections(rng, 480, 640, c) for c in (0, 10, 200, 0, 50)]
        refs = [sr.extract(img, 600, 10, projections=q, radius=8) for img, q in zip(icl, proj)]
        check_sel(run_sel(ctx, sel_params(600, 10), icl, proj, [8] * 5), refs)

        tall = [smooth_noise(rng, 4096, 64, 5)]
        check_fast(po, tall, run_fast(ctx, pg, tall, 2048))

        d0, d1 = first[1][0, :first[3][0]], first[1][1, :first[3][1]]
        got, gflags = ops.bruteforce_match(ctx, ops.bruteforce_params(), d0, d1)
        ref, rflags = oracle.bruteforce_match(d0, d1, 50.0, 0.9)
        assert len(ref) > 50 and corr_equal(ref, got) and gflags == rflags

        small = [smooth_noise(rng, 120, 200, 4) for _ in range(2)]
        refs = [sr.extract(img, 300, 4) for img in small]
        check_sel(run_sel(ctx, sel_params(300, 4), small), refs)

        last = run_fast(ctx, pg, kitti, 2048)
        check_fast(po, kitti, last)
        assert all(np.array_equal(a, b) for a, b in zip(first, last))
    finally:
        ctx.close()
