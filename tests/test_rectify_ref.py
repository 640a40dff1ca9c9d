"""The rectifier's numpy restatement: its float32 parity form against its float64 truth, and ops.stereo_rectification (no GPU)."""
import numpy as np
import pytest

import rectify_ref as ref
from srrg2_proslam_amd import configs, ops

K0 = np.array([[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]])  # EuRoC cam0
D0 = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)


def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def euroc_map():
    cam = configs.EUROC["camera"]
    Kd = np.array([[cam["fx"], 0.0, cam["cx"]], [0.0, cam["fy"], cam["cy"]], [0.0, 0.0, 1.0]])
    return ops.rectify_map(K0, D0, rot(1, 0.01) @ rot(0, 0.007), Kd)


def _compare(img):
    m = euroc_map()
    a, na, _ = ref.rectify(img, m, dtype=np.float32)
    b, nb, _ = ref.rectify(img, m, dtype=np.float64)
    diff = np.abs(a.astype(np.int32) - b.astype(np.int32))
    share = float(np.count_nonzero(diff)) / diff.size
    print("float32 against float64: max %d grey levels, %.4f %% of the pixels differ, border %d / %d" % (diff.max(), 100 * share, na, nb))
    return int(diff.max()), share


def test_float32_against_float64_noise():
    img = np.random.default_rng(0).integers(0, 256, (480, 752)).astype(np.uint8)
    worst, share = _compare(img)
    assert worst <= 1 and share <= 0.005  # the restatement shows 0.15 %: a condition with threefold room, not a tolerance


def test_float32_against_float64_blocks():
    b = np.random.default_rng(0).integers(0, 256, (60, 94)).astype(np.uint8)
    img = np.kron(b, np.ones((8, 8), np.uint8))
    worst, share = _compare(img)
    assert worst <= 1 and share <= 0.0015  # 0.03 % on 8 x 8 blocks


def test_identity_and_shift_are_exact():
    img = np.random.default_rng(1).integers(0, 256, (33, 65)).astype(np.uint8)
    K = np.array([[64.0, 0.0, 30.0], [0.0, 64.0, 16.0], [0.0, 0.0, 1.0]])  # a power of two and integers: every step is exact
    out, nb, st = ref.rectify(img, ops.rectify_map(K, [0] * 5))
    assert np.array_equal(out, img) and nb == 0 and st == 0
    Ks = K.copy()
    Ks[0, 2], Ks[1, 2] = K[0, 2] + 3, K[1, 2] - 2  # dst (u, v) samples src (u + 3, v - 2)
    out, nb, _ = ref.rectify(img, ops.rectify_map(Ks, [0] * 5, None, K), border=7)
    # the shifted image in a frame of border: vs = -2 and -1 (only vs > -1 has a source), us = cols .. cols + 2
    assert np.array_equal(out[2:, :-3], img[:-2, 3:]) and np.all(out[:2] == 7) and np.all(out[:, -3:] == 7)
    assert nb == 2 * 65 + 3 * 31


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_stereo_rectification(seed):
    rng = np.random.default_rng(seed)
    Kl = K0 + np.array([[rng.normal(0, 2), 0, rng.normal(0, 3)], [0, rng.normal(0, 2), rng.normal(0, 3)], [0, 0, 0]])
    Kr = K0 + np.array([[rng.normal(0, 2), 0, rng.normal(0, 3)], [0, rng.normal(0, 2), rng.normal(0, 3)], [0, 0, 0]])
    Dl = np.array(D0) * (1 + rng.normal(0, 0.05, 5))
    Dr = np.array(D0) * (1 + rng.normal(0, 0.05, 5))
    ang = np.deg2rad(rng.uniform(2.0, 3.0))
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R_rl = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    t_rl = np.array([0.11, rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)])
    ml, mr, cam = ops.stereo_rectification(Kl, Dl, Kr, Dr, R_rl, t_rl, (752, 480))
    assert set(cam) == set(configs.EUROC["camera"]) and cam["fx"] == cam["fy"]
    assert abs(cam["baseline_m"] - np.linalg.norm(t_rl)) < 1e-15
    assert abs(cam["fx"] - (Kl[0, 0] + Kl[1, 1] + Kr[0, 0] + Kr[1, 1]) / 4) < 1e-12
    for R in (ml.R, mr.R):
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and np.linalg.det(R) > 0
    # 200 points 1-15 m ahead of the left camera, in its frame; the same points in the right camera's frame
    X_l = np.stack([rng.uniform(-1, 1, 200), rng.uniform(-0.6, 0.6, 200), np.ones(200)], axis=1) * rng.uniform(1, 15, (200, 1))
    X_r = (X_l - t_rl) @ R_rl  # R_rl^T (X_l - t)
    P_l, P_r = X_l @ ml.R.T, X_r @ mr.R.T  # in the two rectified cameras
    uv_l, uv_r = ref.project_distorted(ml, P_l, "dst"), ref.project_distorted(mr, P_r, "dst")
    assert np.max(np.abs(uv_l[:, 1] - uv_r[:, 1])) < 1e-9  # the rows agree
    assert np.max(np.abs((uv_l[:, 0] - uv_r[:, 0]) - cam["fx"] * cam["baseline_m"] / P_l[:, 2])) < 1e-9
    # the map's forward model at the rectified pixel lands on the point's distorted projection in the raw camera
    assert np.max(np.abs(ref.forward_map(ml, uv_l) - ref.project_distorted(ml, X_l))) < 1e-9
    assert np.max(np.abs(ref.forward_map(mr, uv_r) - ref.project_distorted(mr, X_r))) < 1e-9
    # and the fixed-point inverse of the distortion brings those raw pixels back onto the points' rays
    for m, X in ((ml, X_l), (mr, X_r)):
        xy = ref.undistort_points(m, ref.project_distorted(m, X))
        assert np.max(np.abs(xy - X[:, :2] / X[:, 2:])) < 1e-9
