"""The speckle filter's numpy restatement (tests/speckle_ref.py) must not be its own only witness: hand-written images whose
answer is written out here, and an independent flood fill over a Python stack on a few hundred random images.  No GPU needed."""
import numpy as np
import pytest

import speckle_ref as ref

F = np.float32
INF, NAN = F(np.inf), F(np.nan)


def run(image, max_size, max_diff=1.0, companion=None):
    return ref.speckle_image(np.asarray(image), companion, ref.params(max_size, max_diff))


def test_a_2_x_2_block():
    image = np.zeros((4, 5), F)
    image[1:3, 2:4] = 7
    r = run(image, 3)
    assert r["label"].tolist() == [[-1] * 5, [-1, -1, 7, 7, -1], [-1, -1, 7, 7, -1], [-1] * 5]
    assert (r["n_kept"], r["n_removed"]) == (4, 0) and np.array_equal(r["image"], image)
    r = run(image, 4)
    assert (r["n_kept"], r["n_removed"]) == (0, 4) and not r["image"].any() and r["label"][1, 2] == 7  # labels: before removal
    assert (run(image, 0)["n_kept"], run(image, 0)["n_removed"]) == (4, 0)


def test_an_l_and_a_companion():
    image = np.array([[5, 0, 0], [5, 0, 9], [5, 5, 0]], np.uint16)
    companion = np.arange(1, 10, dtype=F).reshape(3, 3)
    r = run(image, 1, companion=companion)
    assert r["label"].tolist() == [[0, -1, -1], [0, -1, 5], [0, 0, -1]]
    assert r["image"].tolist() == [[5, 0, 0], [5, 0, 0], [5, 5, 0]] and (r["n_kept"], r["n_removed"]) == (4, 1)
    assert r["companion"].tolist() == [[1, 2, 3], [4, 5, 0], [7, 8, 9]]  # only the removed pixel; invalid ones keep theirs
    r = run(image, 4, companion=companion)
    assert not r["image"].any() and (r["n_kept"], r["n_removed"]) == (0, 5)
    assert r["companion"].tolist() == [[0, 2, 3], [0, 5, 0], [0, 0, 9]]
    assert image[1, 2] == 9 and companion[1, 2] == 6  # the inputs are not changed


def test_components_that_touch_only_diagonally():
    image = np.array([[3, 0, 3], [0, 3, 0], [3, 0, 3]], F)
    r = run(image, 1)
    assert r["label"].tolist() == [[0, -1, 2], [-1, 4, -1], [6, -1, 8]] and r["n_removed"] == 5
    assert run(image, 0)["n_removed"] == 0


@pytest.mark.parametrize("step", [1.0, 0.75, 1024.0])
def test_ramps(step):
    """k * step is exact for these steps and k <= 8, and so are the differences.  Steps of exactly max_diff connect from end to end,
    whatever the ends differ by; the same steps are nextafter(max_diff, inf) for the float below step, and connect nothing"""
    ramp = (np.arange(1, 9, dtype=F) * F(step)).reshape(1, 8)
    assert (ramp[0, 1:] - ramp[0, :-1] == F(step)).all()
    r = run(ramp, 7, F(step))
    assert r["label"].tolist() == [[0] * 8] and (r["n_kept"], r["n_removed"]) == (8, 0) and run(ramp, 8, F(step))["n_removed"] == 8
    assert run(ramp.T.copy(), 7, F(step))["label"].reshape(-1).tolist() == [0] * 8
    below = np.nextafter(F(step), F(0))
    assert np.nextafter(below, INF) == F(step)
    r = run(ramp, 1, below)
    assert r["label"].tolist() == [list(range(8))] and r["n_removed"] == 8
    assert run(ramp.T.copy(), 1, below)["label"].reshape(-1).tolist() == list(range(8))


def test_a_chain_that_is_not_transitive():
    """1 - 2 - 3: the ends differ by 2 > max_diff and are one component through the middle; side by side they are two"""
    assert run(np.array([[1, 2, 3]], F), 2)["label"].tolist() == [[0, 0, 0]]
    assert run(np.array([[1, 3, 2]], F), 1)["label"].tolist() == [[0, 1, 1]]
    r = run(np.array([[1, 3], [2, 4]], F), 3)
    assert r["label"].tolist() == [[0, 1], [0, 1]] and r["n_removed"] == 4 and run(np.array([[1, 3], [2, 4]], F), 1)["n_removed"] == 0


def test_values_that_are_not_numbers_or_not_positive():
    image = np.array([[1, NAN, 1, INF, INF, 1], [1, -0.0, 1, -1, 0.0, 1]], F)
    r = run(image, 2, max_diff=3e38)
    # NaN, -0, 0 and -1 are invalid; +inf is valid and alone: inf - inf is NaN, inf - 1 is inf
    assert r["label"].tolist() == [[0, -1, 2, 3, 4, 5], [0, -1, 2, -1, -1, 5]]
    assert (r["n_kept"], r["n_removed"]) == (0, 8)
    assert np.array_equal(r["image"], np.array([[0, NAN, 0, 0, 0, 0], [0, -0.0, 0, -1, 0, 0]], F), equal_nan=True)
    assert np.signbit(r["image"][1, 1])  # an invalid pixel is not written: -0 stays -0


def test_the_extremes_of_16_bits():
    image = np.array([[65535, 1, 0, 65535, 65534]], np.uint16)
    assert run(image, 1, 65533)["label"].tolist() == [[0, 1, -1, 3, 3]]
    r = run(image, 1, 65534)
    assert r["label"].tolist() == [[0, 0, -1, 3, 3]] and r["n_removed"] == 0
    assert run(image, 2, 0)["label"].tolist() == [[0, 1, -1, 3, 4]]


def flood_fill(image, max_diff):
    """labels by a depth-first fill over a Python stack: independent of the restatement's propagation"""
    rows, cols = image.shape
    x = image.astype(F)
    valid = image > 0
    label = np.full((rows, cols), -1, np.int32)
    for v0 in range(rows):
        for u0 in range(cols):
            if not valid[v0, u0] or label[v0, u0] >= 0:
                continue
            label[v0, u0] = v0 * cols + u0  # the raster scan meets a component at its least index
            stack = [(v0, u0)]
            while stack:
                v, u = stack.pop()
                for y, z in ((v, u - 1), (v, u + 1), (v - 1, u), (v + 1, u)):
                    if 0 <= y < rows and 0 <= z < cols and valid[y, z] and label[y, z] < 0 and abs(F(x[v, u] - x[y, z])) <= max_diff:
                        label[y, z] = v0 * cols + u0
                        stack.append((y, z))
    return label


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_against_a_flood_fill_on_random_images(dtype):
    rng = np.random.default_rng([20, dtype == np.uint16])
    n = 0
    for case in range(150):
        rows, cols = (int(k) for k in rng.integers(1, 14, 2))
        density = rng.uniform(0.3, 0.7)
        levels = int(rng.integers(1, 5))
        image = (rng.integers(1, levels + 1, (rows, cols)) * (rng.random((rows, cols)) < density)).astype(dtype)
        if dtype == np.float32:
            image *= F(0.5)
            image[rng.random((rows, cols)) < 0.05] = rng.choice([NAN, INF, F(-1), F(-0.0)])
        max_diff = F(rng.choice([0, 0.5, 1, 2] if dtype == np.float32 else [0, 1, 2]))
        with np.errstate(invalid="ignore"):  # inf - inf
            want = flood_fill(image, max_diff)
        assert np.array_equal(ref.labels(image, max_diff), want), case
        valid = want >= 0
        sizes = np.bincount(want[valid], minlength=want.size)
        for max_size in (0, 1, 5, 50, 2 ** 31 - 1):
            r = ref.speckle_image(image, None, ref.params(max_size, max_diff))
            gone = valid & (sizes[np.maximum(want, 0)] <= max_size)
            assert r["n_removed"] == gone.sum() and r["n_kept"] == (valid & ~gone).sum(), (case, max_size)
            assert np.array_equal(r["image"], np.where(gone, dtype(0), image), equal_nan=True) and np.array_equal(r["label"], want)
            assert max_size > 0 or r["n_removed"] == 0
            assert max_size < 2 ** 31 - 1 or r["n_kept"] == 0
            n += int(r["n_removed"] > 0)
    assert n > 300  # the cases do remove something


def test_sequences():
    images = np.ones((2, 2, 2), F)
    r = ref.speckle(images, None, 1, ref.params(4, 0))
    assert r["status"] == 0 and r["results"][1] is None and r["results"][0]["n_removed"] == 4
    for n in (-1, 3):
        assert ref.speckle(images, None, n, ref.params(4, 0)) == dict(status=ref.PRS_ERR_RANGE, results=[None, None])
    assert ref.speckle(images, images, None, ref.params(3, 0))["results"][1]["n_kept"] == 4
