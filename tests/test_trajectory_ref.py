"""The numpy restatement of the trajectory metrics (tests/trajectory_ref.py) on cases with known answers, the time-stamp association
(formats.associate) on hand-made stamps and the benchmark gates (configs.is_regression).  No GPU needed."""
import os

import numpy as np
import pytest

import trajectory_ref as tr
from srrg2_proslam_amd import configs, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


@pytest.fixture(scope="module")
def highway():
    return tr.to44(np.load(os.path.join(ROOT, "tests", "golden", "ref_kitti_gt.npz"))["highway"][:300])


def test_identical_trajectories_give_zero(highway):
    r = tr.evaluate(highway, highway)
    assert r["status"] == 0 and r["n_valid"] == 300 and r["n_rpe"] == 299 and r["n_kitti"] > 0
    for k in ("ate_rmse", "ate_max", "rpe_t_rmse", "rpe_t_max", "rpe_r_rmse", "rpe_r_max", "kitti_t", "kitti_r"):
        assert r[k] <= 1e-9, (k, r[k])
    assert np.all(r["axis_t_mean"] <= 1e-9) and np.all(r["axis_r_std"] <= 1e-9)
    assert np.allclose(r["S"], np.eye(4), atol=1e-9)
    assert np.all(r["frame_error"] >= 0)
    # the path length is the last cumulative distance
    assert abs(r["path_length"] - np.linalg.norm(np.diff(highway[:, :3, 3], axis=0), axis=1).sum()) < 1e-9


def test_fixed_transform_is_undone_by_the_rigid_alignment(highway):
    T = pose(rot([0.3, -1.0, 0.2], 2.5), [1000.0, -20.0, 300.0])
    P = T @ highway  # float64 product, rounded to float32 by the evaluator: ~1e-4 m at 1 km
    r = tr.evaluate(P, highway, align=tr.ALIGN_RIGID)
    assert r["ate_rmse"] < 5e-4 and r["ate_max"] < 2e-3
    assert np.allclose(r["S"], np.linalg.inv(T), atol=2e-3)
    assert np.allclose(r["S"][:3, :3], np.linalg.inv(T)[:3, :3], atol=1e-5)
    assert abs(np.linalg.det(r["S"][:3, :3]) - 1.0) < 1e-12
    # a relative pose does not see a transform applied on the left
    assert r["rpe_t_rmse"] < 1e-3 and r["rpe_r_rmse"] < 1e-5
    # FIRST undoes it from one row, NONE leaves it
    assert tr.evaluate(P, highway, align=tr.ALIGN_FIRST)["ate_rmse"] < 2e-2
    assert tr.evaluate(P, highway, align=tr.ALIGN_NONE)["ate_mean"] > 500.0


def test_constant_drift_is_the_relative_error(highway):
    D = pose(rot([0, 0, 1], 0.004), [0.03, 0.0, 0.04])  # per frame: 0.05 m, 0.004 rad
    P, cur = [], np.eye(4)
    for k in range(highway.shape[0]):
        P.append(cur.copy())
        cur = cur @ D
    G = np.stack([np.eye(4)] * highway.shape[0])  # the ground truth stands still: E = D for every pair
    r = tr.evaluate(np.stack(P), G, align=tr.ALIGN_FIRST, kitti_step=0)
    assert r["n_rpe"] == highway.shape[0] - 1 and r["n_kitti"] == 0
    for k in ("rpe_t_rmse", "rpe_t_mean", "rpe_t_max"):
        assert abs(r[k] - 0.05) < 1e-6, (k, r[k])
    for k in ("rpe_r_rmse", "rpe_r_mean", "rpe_r_max"):
        assert abs(r[k] - 0.004) < 1e-6, (k, r[k])
    assert np.allclose(r["axis_t_mean"], [0.03, 0.0, 0.04], atol=1e-6)
    assert np.allclose(r["axis_r_mean"], [0.0, 0.0, np.degrees(0.004)], atol=1e-4)
    assert np.all(r["axis_t_std"] < 1e-6) and np.all(r["axis_r_std"] < 1e-4)
    # ten frames apart the drift composes: ten times the angle
    r10 = tr.evaluate(np.stack(P), G, align=tr.ALIGN_FIRST, rpe_delta=10, kitti_step=0)
    assert abs(r10["rpe_r_mean"] - 0.04) < 1e-6 and r10["n_rpe"] == highway.shape[0] - 10


def test_small_angles_keep_their_digits():
    th, rv = tr.rotation_vector(rot([1, 2, 3], 1e-7))
    assert abs(th - 1e-7) < 1e-20 * 1e7 and abs(np.linalg.norm(rv) - 1e-7) < 1e-13
    th, rv = tr.rotation_vector(np.eye(3))
    assert th == 0.0 and np.all(rv == 0.0)


def test_mirrored_planar_cloud_gets_a_proper_rotation():
    rng = np.random.default_rng(5)
    g = np.zeros((40, 3))
    g[:, :2] = rng.uniform(-50, 50, (40, 2))
    p = g * np.array([1.0, -1.0, 1.0])  # mirrored in the plane: a half turn about x brings it back
    S = tr.rigid_alignment(p, g)
    assert abs(np.linalg.det(S[:3, :3]) - 1.0) < 1e-12
    assert np.allclose(S[:3, :3] @ S[:3, :3].T, np.eye(3), atol=1e-12)
    assert np.abs(g - (p @ S[:3, :3].T + S[:3, 3])).max() < 1e-9
    # slightly out of the plane the unconstrained optimum is a reflection: still a rotation, and the residual is what is left
    g2 = g.copy()
    g2[:, 2] = rng.uniform(-0.5, 0.5, 40)
    S2 = tr.rigid_alignment(g2 * np.array([1.0, -1.0, 1.0]), g2)
    assert abs(np.linalg.det(S2[:3, :3]) - 1.0) < 1e-12


def test_masks_and_short_sequences(highway):
    valid = np.ones(300, np.uint8)
    valid[::2] = 0
    r = tr.evaluate(highway, highway, valid=valid)
    assert r["n_valid"] == 150 and r["n_rpe"] == 0 and r["n_kitti"] == 0 and r["path_length"] == 0.0
    assert np.all(r["frame_error"][::2] == -1) and np.all(r["frame_error"][1::2] >= 0)
    assert tr.evaluate(highway, highway, valid=valid, rpe_delta=2)["n_rpe"] == 149
    for n, want in ((0, -4), (2, -4), (3, 0)):
        assert tr.evaluate(highway, highway, n_frames=n)["status"] == want
    assert tr.evaluate(highway, highway, n_frames=0, align=tr.ALIGN_NONE)["status"] == 0
    assert tr.evaluate(highway, highway, n_frames=0, align=tr.ALIGN_FIRST)["status"] == -4
    assert tr.evaluate(highway, highway, n_frames=-1, align=tr.ALIGN_NONE)["status"] == -4


def test_associate():
    est = [0.00, 0.10, 0.20, 0.30, 0.50]
    gt = [0.011, 0.105, 0.1001, 0.215, 0.281, 0.9]
    rows, valid = formats.associate(est, gt, 0.02)
    # 0.10 takes 0.1001 (nearer than 0.105); 0.30 takes 0.281 (0.019 off); 0.50 has nothing within 0.02
    assert rows.tolist() == [0, 2, 3, 4, -1] and valid.tolist() == [1, 1, 1, 1, 0]
    # one ground-truth stamp serves one row: the nearer claim wins, the other row goes without
    rows, valid = formats.associate([1.00, 1.01], [1.008], 0.02)
    assert rows.tolist() == [-1, 0] and valid.tolist() == [0, 1]
    # the bound is strict, as TUM's
    assert formats.associate([0.0], [0.02], 0.02)[1].tolist() == [0]
    rows, valid = formats.associate([], [1.0])
    assert rows.size == 0 and valid.size == 0


def test_benchmark_gates():
    assert sorted(configs.BENCHMARK_GATES) == ["euroc", "icl", "kitti", "malaga", "tum"]
    g = configs.BENCHMARK_GATES["kitti"]
    assert g["mean_translation"] == (0.3,) * 3 and g["std_translation"] == (1.0,) * 3
    assert g["mean_rotation"] == (3,) * 3 and g["std_rotation"] == (3,) * 3 and g["source"].endswith("benchmark_kitti.cpp:17-20")
    assert configs.BENCHMARK_GATES["icl"]["mean_translation"] == (0.02,) * 3
    assert configs.BENCHMARK_GATES["malaga"]["std_translation"] == (10,) * 3
    ok = dict(status=0, n_rpe=10, axis_t_mean=np.array([0.1, 0.2, 0.3]), axis_t_std=np.zeros(3), axis_r_mean=np.ones(3), axis_r_std=np.ones(3))
    assert not configs.is_regression(ok, "kitti")
    assert configs.is_regression(ok, "icl")
    assert configs.is_regression(dict(ok, axis_r_std=np.array([0.0, 3.5, 0.0])), g)
    assert configs.is_regression(dict(ok, axis_t_mean=np.array([np.nan, 0, 0])), g)
    assert configs.is_regression(dict(ok, n_rpe=0), g) and configs.is_regression(dict(ok, status=-4), g)
