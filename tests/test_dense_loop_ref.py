"""The dense tracker's loop restated (tests/dense_loop_ref.py) against the true trajectory and the true scene, on the cases of
tests/dense_loop_cases.py: two trajectories of eight 80 x 60 frames in a turned world frame, 4 cm voxels, both depth types.  No GPU
needed; tests/test_dense_loop_gpu.py compares ops.DenseTrackerBatch with this restatement byte for byte and holds the device's own
poses, mesh and view to the bounds below.

Measured with this restatement (x86-64, numpy 2, glibc libm), every figure the range over A / B and f32 / u16:

  pose error per step     2.0 .. 5.39 mm, 0.56 .. 2.35 mrad; it grows with k, the worst is A u16 at step 7 (A f32: 5.34 mm, 2.34 mrad;
                          B f32: 4.09 mm, 1.57 mrad; B u16: 3.86 mm, 1.45 mrad at step 7).       Bounds: twice the worst.
  inliers of a step       2955 .. 3793 of 4800 samples, 10 steps taken, status 1.                 Bound: more than 2500.
  B, the empty frame 3    status 0, 0 inliers, 0 steps, pose 3 = pose 2, the volume's bytes stay (26.7 mm, 22.3 mrad from the truth:
                          the one step left out of the bound); step 4 sees twice the increment and leaves 2.72 / 2.61 mm,
                          0.97 / 0.89 mrad.
  wrong compositions      A f32 at step 1: X * pose 112.6 mm, 21.5 mrad; pose * X^-1 54.3 mm, 43.0 mrad; pose kept 27.7 mm, 21.7 mrad
                          (the tracker's own: 2.42 mm, 0.87 mrad).                                Floors: 50, 25 and 15 mm.
  the mesh                5874 .. 6456 vertices, 5409 .. 6024 quads, status 0, a normal on every vertex; distance to the scene in
                          voxels: mean 0.0496 .. 0.0511, 99th percentile 0.2662 .. 0.2671, max 0.4765 .. 0.4996.
                                                                                                  Bounds: 0.1, 0.5 and 1.0.
  the mesh's normals      cosine with the scene's normal: 5th percentile 0.9057 .. 0.9303 (the minimum, 0.297 .. 0.406, lies in the
                          creases where two planes meet and is not bounded), none negative.       Bounds: 0.856 (0.906 - 0.05), none.
  the view from the truth the volume raycast at the true last pose against the analytic depth: coverage 0.7817 .. 0.8179, mean error
                          0.1389 .. 0.1593 voxels, 0.0051 .. 0.0069 of the errors over a voxel.   Bounds: 0.7, 0.3 and 0.02.

The margin of two on the pose covers libm and numpy differences in `offset` and `render`, not the device: the device is compared
with the restatement byte for byte."""
import numpy as np
import pytest

import dense_align_cases
import dense_align_ref
import dense_loop_cases as cases
import dense_loop_ref as loop

F = np.float32
MAX_TRANSLATION, MAX_ROTATION = 1.08e-2, 4.7e-3          # twice 5.39 mm and 2.35 mrad
MIN_INLIERS, STEPS = 2500, 10
UNBOUNDED = {("B", 3)}                                   # the one step left out of the pose bound: the empty frame
MUTANT_FLOORS = {"X * pose": 0.050, "pose * X^-1": 0.025, "pose kept": 0.015}
MAP_MEAN, MAP_P99, MAP_MAX, MAP_COS_P5 = 0.1, 0.5, 1.0, 0.856
VIEW_COVERAGE, VIEW_MEAN, VIEW_OVER = 0.7, 0.3, 0.02
RUNS = [(name, depth_type) for name in sorted(cases.TRAJECTORIES) for depth_type in cases.DEPTH_TYPES]


def check_poses(name, poses, what=""):
    """poses [FRAMES, 4, 4] of a tracked trajectory against the truth: every step but the unbounded one within the bound
    -> the errors [(metres, radians)]"""
    truth = cases.true_poses(name)
    errors = [dense_align_ref.pose_error(poses[k], truth[k]) for k in range(cases.FRAMES)]
    print("%s %s: %s" % (what, name, " ".join("%.2f mm %.2f mrad," % (1e3 * dt, 1e3 * dr) for dt, dr in errors[1:])))
    for k, (dt, dr) in enumerate(errors):
        if (name, k) not in UNBOUNDED:
            assert dt <= MAX_TRANSLATION and dr <= MAX_ROTATION, (what, name, k, dt, dr)
    return errors


def check_map(vertex, normal, what=""):
    """a mesh's vertices and normals [n, 4] in the world against the scene -> the measurements"""
    vertex, normal = np.asarray(vertex), np.asarray(normal)
    assert len(vertex) > 5000 and (normal[:, 3] == 1).all(), what                    # a normal on every vertex
    distance, scene_normal = cases.scene_distance(cases.to_local(vertex[:, :3]))
    distance = distance / cases.VS
    cos = ((normal[:, :3].astype(np.float64) @ cases.G[:3, :3]) * scene_normal).sum(1)
    m = dict(mean=distance.mean(), p99=np.percentile(distance, 99), max=distance.max(), cos_p5=np.percentile(cos, 5), cos_min=cos.min(),
             negative=float((cos < 0).mean()))
    print("%s map: %d vertices, %s" % (what, len(vertex), ", ".join("%s %.4f" % kv for kv in m.items())))
    assert m["mean"] <= MAP_MEAN and m["p99"] <= MAP_P99 and m["max"] <= MAP_MAX, (what, m)
    assert m["cos_p5"] >= MAP_COS_P5 and m["negative"] == 0, (what, m)
    return m


def check_view(name, depth, what=""):
    """a raycast of a tracked volume at the true last pose, depth [ROWS, COLS], against the analytic depth -> the measurements"""
    want = dense_align_cases.render(cases.local_poses(name)[-1])[0]
    depth = np.asarray(depth)
    seen = want > 0
    hit = seen & (depth > 0)
    error = np.abs(depth[hit].astype(np.float64) - want[hit]) / cases.VS
    m = dict(coverage=hit.sum() / seen.sum(), mean=error.mean(), over=float((error > 1).mean()))
    print("%s view: %s" % (what, ", ".join("%s %.4f" % kv for kv in m.items())))
    assert m["coverage"] >= VIEW_COVERAGE and m["mean"] <= VIEW_MEAN and m["over"] <= VIEW_OVER, (what, m)
    return m


def test_the_cases_are_the_turned_scene():
    """G is a rigid quarter turn; the turned box is the box of tests/test_dense_align_gpu.py; a frame moves 2.5 to 3 cm and 1 to 1.5
    degrees; the empty frame is B's third alone"""
    R = cases.G[:3, :3]
    assert (R @ R.T == np.eye(3)).all() and np.linalg.det(R) == 1 and cases.G[:3, 3].tolist() == [4.0, -2.0, 7.0]
    lo = np.array([-1.4, -1.1, 1.1])
    corners = np.array([lo, lo + np.array([70, 55, 60]) * cases.VS]) @ R.T + cases.G[:3, 3]
    assert np.allclose(corners.min(0), cases.ORIGIN[:3], atol=1e-12)
    assert np.allclose(corners.max(0) - corners.min(0), np.array(cases.DIMS) * cases.VS, atol=1e-12)
    for name in cases.TRAJECTORIES:
        truth = cases.true_poses(name)
        for k in range(1, cases.FRAMES):
            dt, dr = dense_align_ref.pose_error(truth[k], truth[k - 1])
            assert 0.025 < dt < 0.03 and 0.018 < dr < 0.026, (name, k, dt, dr)
        for depth_type in cases.DEPTH_TYPES:
            f = cases.frames(name, depth_type)
            assert f.dtype == (F if depth_type == "f32" else np.uint16) and f.shape == (cases.FRAMES, cases.ROWS, cases.COLS)
            assert [k for k in range(cases.FRAMES) if not f[k].any()] == list(cases.EMPTY[name])
            assert all(((f[k] > 0).mean() == 1.0) for k in range(cases.FRAMES) if k not in cases.EMPTY[name])
    assert cases.EMPTY == {"A": (), "B": (3,)} and UNBOUNDED == {("B", 3)}


def test_scene_distance_on_points_of_the_scene():
    """points rendered on the scene lie on it, their normals are the rendered ones; a point pushed along its normal lies that far off"""
    P = cases.local_poses("A")[2]
    depth, normal = dense_align_cases.render(P)
    v, u = np.meshgrid(np.arange(cases.ROWS), np.arange(cases.COLS), indexing="ij")
    cam = cases.CAMERA
    d = depth.astype(np.float64)
    points = np.stack([(u - cam["cx"]) / cam["fx"] * d, (v - cam["cy"]) / cam["fy"] * d, d], -1).reshape(-1, 3) @ P[:3, :3].T + P[:3, 3]
    distance, n = cases.scene_distance(points)
    assert distance.max() < 1e-6                                   # float32 depths
    rendered = normal[..., :3].reshape(-1, 3).astype(np.float64) @ P[:3, :3].T
    crease = np.sort(cases.surface_distances(points)[0], axis=0)[1] < 1e-3            # a second surface as near: either normal is right
    assert ((n * rendered).sum(1)[~crease] > 1 - 1e-6).all() and crease.mean() < 0.02      # towards the room = towards the camera
    off, _ = cases.scene_distance(points + 0.01 * n)
    alone = np.sort(cases.surface_distances(points)[0], axis=0)[1] > 0.03             # no second surface within reach of the push
    assert np.allclose(off[alone], 0.01, atol=1e-6) and alone.mean() > 0.8
    world = points @ cases.G[:3, :3].T + cases.G[:3, 3]
    assert np.allclose(cases.to_local(world), points, atol=1e-12)


@pytest.mark.parametrize("name,depth_type", RUNS)
def test_the_restated_loop_follows_the_true_trajectory(name, depth_type):
    steps, _ = loop.tracked(name, depth_type)
    check_poses(name, [s["pose"] for s in steps], depth_type)
    for k in range(1, cases.FRAMES):
        r = steps[k]["result"]
        if k in cases.EMPTY[name]:
            continue
        assert (r["status"], r["steps_taken"], r["iterations"]) == (1, STEPS, STEPS) and r["num_inliers"] > MIN_INLIERS, (k, r)
        assert steps[k]["n_updates"] > 50000 and steps[k]["volume"] != steps[k - 1]["volume"]
        assert steps[k]["pose"].tobytes() != steps[k - 1]["pose"].tobytes()


@pytest.mark.parametrize("depth_type", cases.DEPTH_TYPES)
def test_a_frame_that_cannot_be_aligned_keeps_the_pose_and_the_volume(depth_type):
    steps, _ = loop.tracked("B", depth_type)
    r = steps[3]["result"]
    assert (r["status"], r["num_inliers"], r["steps_taken"]) == (0, 0, 0) and r["num_unmatched"] == r["num_samples"] == 4800
    assert steps[3]["X"].tobytes() == np.eye(4, dtype=F).tobytes() and not steps[3]["mask"].any()
    assert steps[3]["pose"].tobytes() == steps[2]["pose"].tobytes()
    assert steps[3]["n_updates"] == 0 and steps[3]["volume"] == steps[2]["volume"]
    # the next frame is aligned from a pose two increments back, within the same bound
    truth = cases.true_poses("B")
    start = dense_align_ref.pose_error(steps[3]["pose"], truth[4])
    assert start[0] > 0.05 and start[1] > 0.04
    dt, dr = dense_align_ref.pose_error(steps[4]["pose"], truth[4])
    print("B %s step 4: %.3g m, %.3g rad left" % (depth_type, dt, dr))
    assert dt <= MAX_TRANSLATION and dr <= MAX_ROTATION and steps[4]["result"]["steps_taken"] == STEPS


@pytest.mark.parametrize("mutant", sorted(MUTANT_FLOORS))
def test_the_scene_tells_a_wrong_composition_apart(mutant):
    """the evidence that the bound sees a tracker that composes X on the wrong side, inverted or not at all: each misses it at
    step 1 by at least its floor, which is itself well beyond the bound"""
    floor = MUTANT_FLOORS[mutant]
    assert floor > 1.3 * MAX_TRANSLATION
    steps, _ = loop.tracked("A", "f32", mutant, 2)
    dt, dr = dense_align_ref.pose_error(steps[1]["pose"], cases.true_poses("A")[1])
    print("%s: %.3g m, %.3g rad left" % (mutant, dt, dr))
    assert dt >= floor, (mutant, dt, dr)
    right = loop.tracked("A", "f32")[0][1]
    assert steps[1]["X"].tobytes() == right["X"].tobytes() and steps[1]["pose"].tobytes() != right["pose"].tobytes()


@pytest.mark.parametrize("name,depth_type", RUNS)
def test_the_tracked_volume_meshes_onto_the_scene(name, depth_type):
    m = loop.mesh_of(name, depth_type)
    assert m["status"] == 0 and m["n_vertices"] == m["n_vertices_total"] and m["n_quads"] == m["n_quads_total"] > 5000
    check_map(m["vertex"][:m["n_vertices"]], m["normal"][:m["n_vertices"]], "%s %s" % (name, depth_type))


@pytest.mark.parametrize("name,depth_type", RUNS)
def test_the_tracked_volume_seen_from_the_true_last_pose(name, depth_type):
    view = loop.view_of(name, depth_type)
    assert view["status"] == 0 and view["n_skipped"] == 0
    check_view(name, view["depth"][0], "%s %s" % (name, depth_type))
