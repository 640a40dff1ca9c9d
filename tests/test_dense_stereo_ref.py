"""The numpy restatement of the dense stereo stage (tests/dense_stereo_ref.py) against things it cannot have copied: a random-dot
stereogram with planted disparities, constant images, a scalar triple-loop implementation of the rule written here in Python ints and
float64, and the reference's SceneFlow pair with its sparse ground truth.  No GPU needed; the device is compared with the
restatement byte for byte in tests/test_dense_stereo_gpu.py."""
import os

import numpy as np
import pytest

import dense_stereo_ref as ref

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_random_dot_stereogram():
    """planted disparity 3 everywhere, 9 inside rows 10..29 x columns 30..69: left(y, x) = right(y, x - d)"""
    rng = np.random.default_rng(7)
    right = rng.integers(0, 256, (40, 96), dtype=np.uint8)
    xs = np.arange(96)
    left = right[:, np.clip(xs - 3, 0, 95)].copy()
    left[10:30, 30:70] = right[10:30, np.clip(np.arange(30, 70) - 9, 0, 95)]
    out = ref.dense_stereo_image(left, right, ref.params(100.0, n_disparities=16, aggregation_radius=2, uniqueness_percent=10, lr_max_diff=1))
    d = out["disparity"]
    inner = d[14:26, 36:60]
    assert (inner > 0).all() and np.abs(inner - 9).max() <= 0.5, (float((inner > 0).mean()), float(np.abs(inner - 9).max()))
    for cols in (slice(22, 26), slice(80, 92)):
        outer = d[:, cols]
        assert (outer > 0).all() and np.abs(outer - 3).max() <= 0.5, (cols, float((outer > 0).mean()), float(np.abs(outer - 3).max()))
    valid = d > 0
    assert out["n_valid"] == int(valid.sum()) and (out["depth"][~valid] == 0).all()
    assert (out["depth"][valid] == F(100.0) / d[valid]).all()


def test_constant_images():
    """all costs equal: the strict uniqueness test rejects every pixel; without it the lowest admissible disparity wins"""
    c = np.full((12, 20), 77, np.uint8)
    for q in (1, 10, 99):
        out = ref.dense_stereo_image(c, c, ref.params(50.0, 8, 0, 1, q, 1))
        assert out["n_valid"] == 0 and not out["disparity"].any() and not out["depth"].any()
    out = ref.dense_stereo_image(c, c, ref.params(50.0, 8, 1, 1, 0, 1))
    assert (out["disparity"][:, 1:] == 1.0).all() and (out["disparity"][:, 0] == 0.0).all()
    assert (out["depth"][:, 1:] == 50.0).all() and out["n_valid"] == 12 * 19


def scalar_dense_stereo(left, right, p):
    """rules 1 to 9 pixel by pixel: Python ints, float64 for the two divisions (exact in float32's range of integers, then rounded
    once to float32, which is the correctly rounded float32 quotient)"""
    rows, cols = left.shape
    n, d0, r, q, lr = p["n_disparities"], p["min_disparity"], p["aggregation_radius"], p["uniqueness_percent"], p["lr_max_diff"]
    cy = lambda y: min(max(y, 0), rows - 1)  # noqa: E731
    cx = lambda x: min(max(x, 0), cols - 1)  # noqa: E731

    def census(I, y, x):
        bits = []
        for dy in range(-3, 4):
            for dx in range(-4, 5):
                if (dy, dx) != (0, 0):
                    bits.append(int(I[cy(y + dy), cx(x + dx)]) < int(I[y, x]))
        return bits

    cl = [[census(left, y, x) for x in range(cols)] for y in range(rows)]
    cr = [[census(right, y, x) for x in range(cols)] for y in range(rows)]
    ham = lambda a, b: sum(i != j for i, j in zip(a, b))  # noqa: E731

    def agg(v, u, d, right_ref):
        s = 0
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                y, x = cy(v + dy), cx(u + dx)
                s += ham(cr[y][x], cl[y][min(x + d, cols - 1)]) if right_ref else ham(cl[y][x], cr[y][max(x - d, 0)])
        return s

    def win(v, u, right_ref):
        costs = {d: agg(v, u, d, right_ref) for d in range(d0, d0 + n) if (u + d <= cols - 1 if right_ref else u - d >= 0)}
        if not costs:
            return None, costs
        best = min(costs, key=lambda d: (costs[d], d))
        return best, costs

    disparity, depth = np.zeros((rows, cols), F), np.zeros((rows, cols), F)
    for v in range(rows):
        for u in range(cols):
            d, costs = win(v, u, False)
            if d is None:
                continue
            far = [c for e, c in costs.items() if abs(e - d) >= 2]
            if q > 0 and far and not 100 * costs[d] < (100 - q) * min(far):
                continue
            if lr >= 0:
                dr, _ = win(v, u - d, True)
                if dr is None or abs(dr - d) > lr:
                    continue
            delta = F(0)
            if d - 1 >= d0 and d + 1 <= d0 + n - 1 and d + 1 in costs:
                den = costs[d - 1] + costs[d + 1] - 2 * costs[d]
                if den > 0:
                    delta = F(np.float64(costs[d - 1] - costs[d + 1]) / np.float64(2 * den))
            s = F(F(d) + delta)
            if s > 0:
                disparity[v, u] = s
                depth[v, u] = F(np.float64(p["bf"]) / np.float64(s))
    return disparity, depth


@pytest.mark.parametrize("kw", [dict(n_disparities=6, min_disparity=0, aggregation_radius=1, uniqueness_percent=10, lr_max_diff=1),
                                dict(n_disparities=5, min_disparity=1, aggregation_radius=2, uniqueness_percent=0, lr_max_diff=0),
                                dict(n_disparities=16, min_disparity=0, aggregation_radius=0, uniqueness_percent=30, lr_max_diff=-1)])
def test_brute_force_scalar(kw):
    rng = np.random.default_rng([11, kw["n_disparities"]])
    right = rng.integers(0, 256, (9, 14), dtype=np.uint8)
    left = right[:, np.clip(np.arange(14) - 2, 0, 13)].copy()
    left[rng.random(left.shape) < 0.2] = rng.integers(0, 256)  # some pixels disagree: near-ties and rejected pixels
    p = ref.params(F(718.856) * F(0.537166), **kw)
    out = ref.dense_stereo_image(left, right, p)
    disparity, depth = scalar_dense_stereo(left, right, p)
    assert out["disparity"].tobytes() == disparity.tobytes()
    assert out["depth"].tobytes() == depth.tobytes()
    assert 0 < out["n_valid"] == int((disparity > 0).sum()) < 9 * 14


def test_scene_flow_pair():
    """the reference's SceneFlow pair against its sparse ground truth (row, column, row, right column, disparity; the first entry of
    a pixel counts, as in ref_pins.scene_flow_inliers), scored on the ground-truth pixels of disparity <= 126.  The conditions: at
    least 40 % valid and 55 % of the valid within 1 px.  The four counts are this restatement's own, pinned: the device reproduces
    them because its images are byte-identical"""
    z = np.load(os.path.join(GOLDEN, "ref_scene_flow.npz"))
    out = ref.dense_stereo_image(z["left"], z["right"], ref.params(1.0, 128, 0, 3, 10, 1))
    d = out["disparity"]
    got = {}
    for name in ("gt_threshold_10", "gt_threshold_100"):
        gt = {}
        for r, c, _, _, disp in z[name]:
            gt.setdefault((int(r), int(c)), float(disp))
        scored = [(k, v) for k, v in gt.items() if v <= 126]
        valid = [(k, v) for k, v in scored if d[k] > 0]
        good = sum(abs(float(d[k]) - v) <= 1.0 for k, v in valid)
        assert len(valid) >= 0.40 * len(scored) and good >= 0.55 * len(valid), (name, len(scored), len(valid), good)
        got[name] = (len(scored), len(valid), good)
    assert got == {"gt_threshold_10": (8749, 4394, 2867), "gt_threshold_100": (637, 363, 260)}
    assert out["n_valid"] == 207591
