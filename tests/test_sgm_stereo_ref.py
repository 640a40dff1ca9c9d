"""The numpy restatement of semi-global dense stereo (tests/sgm_stereo_ref.py) against a plain scalar recursion written here, the
properties the rule has by construction (zero penalties, one disparity, flips), and what the path aggregation is for: a textureless
wall that the local rule (tests/dense_stereo_ref.py) rejects whole is filled, and the real crops keep more pixels.  No GPU needed."""
import numpy as np
import pytest

import dense_stereo_ref as dref
import sgm_stereo_ref as ref

F = np.float32


def _rng(*seed):
    return np.random.default_rng(list(seed))


def shifted_pair(rng, rows, cols, shift=3):
    right = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    left = right[:, np.clip(np.arange(cols) - shift, 0, cols - 1)].copy()
    redraw = rng.random((rows, cols)) < 0.1
    left[redraw] = rng.integers(0, 256, int(redraw.sum()), dtype=np.uint8)
    return left, right


def scalar_aggregate(C, n_paths, p1, p2):
    """S by the recursion as the header states it, a pixel and a disparity at a time, every path from its own border pixels"""
    rows, cols, n = C.shape
    S = np.zeros((rows, cols, n), np.int64)
    for dy, dx in ref.PATHS[n_paths]:
        L = np.zeros((rows, cols, n), np.int64)
        for y in (range(rows) if dy >= 0 else range(rows - 1, -1, -1)):
            for x in (range(cols) if dx >= 0 else range(cols - 1, -1, -1)):
                qy, qx = y - dy, x - dx
                for i in range(n):
                    if not (0 <= qy < rows and 0 <= qx < cols):
                        L[y, x, i] = C[y, x, i]
                        continue
                    m = min(L[qy, qx, k] for k in range(n))
                    terms = [L[qy, qx, i], m + p2]
                    if i - 1 >= 0:
                        terms.append(L[qy, qx, i - 1] + p1)
                    if i + 1 <= n - 1:
                        terms.append(L[qy, qx, i + 1] + p1)
                    L[y, x, i] = C[y, x, i] + min(terms) - m
        S += L
    return S


@pytest.mark.parametrize("penalties", [(0, 0), (3, 3), (2, 9)])
@pytest.mark.parametrize("n_paths", [4, 8])
@pytest.mark.parametrize("rows,cols,n", [(7, 9, 5), (1, 6, 3), (6, 1, 2), (5, 4, 1), (4, 7, 4)])
def test_the_restatement_equals_a_scalar_recursion(rows, cols, n, n_paths, penalties):
    left, right = shifted_pair(_rng(1, rows, cols, n), rows, cols, shift=1)
    C = ref.raw_cost(ref.census(left), ref.census(right), 1 + np.arange(n))
    S, _ = ref.aggregate(C, n_paths, *penalties)
    assert np.array_equal(S, scalar_aggregate(C, n_paths, *penalties))


PROPERTY = dict(rows=19, cols=45, n_disparities=13, min_disparity=1)


def property_pair():
    return shifted_pair(_rng(2), PROPERTY["rows"], PROPERTY["cols"], shift=4)


@pytest.mark.parametrize("n_paths", [4, 8])
def test_zero_penalties_sum_the_raw_cost(n_paths):
    left, right = property_pair()
    C = ref.raw_cost(ref.census(left), ref.census(right), 1 + np.arange(13))
    S, top = ref.aggregate(C, n_paths, 0, 0)
    assert np.array_equal(S, n_paths * C) and top == C.max()


@pytest.mark.parametrize("n_paths", [4, 8])
def test_one_disparity_sums_the_raw_cost(n_paths):
    left, right = property_pair()
    C = ref.raw_cost(ref.census(left), ref.census(right), np.array([3]))
    S, _ = ref.aggregate(C, n_paths, 10, 120)
    assert np.array_equal(S, n_paths * C)


@pytest.mark.parametrize("n_paths", [4, 8])
def test_flipping_both_images_top_to_bottom_flips_the_outputs(n_paths):
    left, right = property_pair()
    p = ref.params(20.0, 13, 1, 10, 120, n_paths, 10, 1)
    a = ref.sgm_stereo_image(left, right, p, details=True)
    b = ref.sgm_stereo_image(left[::-1], right[::-1], p, details=True)
    assert a["n_valid"] == b["n_valid"] > 0.5 * 19 * 41 and np.array_equal(a["S"], b["S"][::-1])
    for k in ("disparity", "depth"):
        assert a[k].tobytes() == np.ascontiguousarray(b[k][::-1]).tobytes(), k


def test_path_costs_pass_a_byte():
    """what an 8-bit path cost cannot hold; S itself stays below the "no cost" value"""
    left, right = property_pair()
    out = ref.sgm_stereo_image(left, right, ref.params(20.0, 13, 1, 4095, 4095, 4), details=True)
    assert out["max_path_cost"] > 255 and out["S"].max() < 0xffff


def wall():
    rng = np.random.default_rng(5)
    scene = rng.integers(0, 256, (24, 100), dtype=np.uint8)
    scene[:, 34:66] = 128
    return np.ascontiguousarray(scene[:, :96]), np.ascontiguousarray(scene[:, 4:])  # left, right: disparity 4 everywhere


BAND = (slice(None), slice(42, 54))


def test_the_local_rule_rejects_the_textureless_wall():
    left, right = wall()
    out = dref.dense_stereo_image(left, right, dref.params(20.0, 16, 0, 3, 10, 1))
    assert out["disparity"][BAND].size == 288 and int((out["disparity"][BAND] > 0).sum()) == 0


@pytest.mark.parametrize("n_paths", [4, 8])
@pytest.mark.parametrize("penalties", [(10, 120), (7, 86)])
def test_path_aggregation_fills_the_textureless_wall(penalties, n_paths):
    left, right = wall()
    out = ref.sgm_stereo_image(left, right, ref.params(20.0, 16, 0, penalties[0], penalties[1], n_paths, 10, 1))
    band = out["disparity"][BAND]
    assert int((band > 0).sum()) == 288 and (np.abs(band - 4) <= 0.5).all()


@pytest.mark.parametrize("n_paths", [4, 8])
def test_without_penalties_the_wall_stays_empty(n_paths):
    left, right = wall()
    out = ref.sgm_stereo_image(left, right, ref.params(20.0, 16, 0, 0, 0, n_paths, 10, 1))
    assert int((out["disparity"][BAND] > 0).sum()) == 0


def crops():
    import ref_pins as rp
    from srrg2_proslam_amd import configs
    sf = rp.load("ref_scene_flow")
    crop = lambda image, r0, c0, rows, cols: np.ascontiguousarray(image[r0:r0 + rows, c0:c0 + cols])  # noqa: E731
    bf = lambda cam: F(np.float64(cam["fx"]) * np.float64(cam["baseline_m"]))  # noqa: E731
    return {"scene flow": (crop(sf["left"], 200, 224, 128, 512), crop(sf["right"], 200, 224, 128, 512), 0, F(20.0), 0.5),
            "kitti": (crop(rp.kitti_image("left", 0), 140, 420, 96, 400), crop(rp.kitti_image("right", 0), 140, 420, 96, 400), 1,
                      bf(configs.KITTI["camera"]), 0.7)}


@pytest.mark.parametrize("name", ["scene flow", "kitti"])
def test_real_crops_keep_more_pixels_than_the_local_rule(name):
    left, right, d0, bf, share = crops()[name]
    local = dref.dense_stereo_image(left, right, dref.params(bf, 128, d0, 3, 10, 1))["n_valid"]
    for n_paths in (4, 8):
        got = ref.sgm_stereo_image(left, right, ref.params(bf, 128, d0, 10, 120, n_paths, 10, 1))["n_valid"]
        print(name, "local", local, "sgm", n_paths, "paths", got, "of", left.size)
        assert got > local and got > share * left.size, (name, n_paths, got, local)
