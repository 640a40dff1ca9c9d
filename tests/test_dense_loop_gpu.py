"""ops.DenseTrackerBatch in a closed loop on the device, on the cases of tests/dense_loop_cases.py: a batch of three sequences
(trajectory A, trajectory B with its empty frame, trajectory A again) tracked for eight frames in a turned world frame, where a pose
composed on the wrong side, inverted or not at all lies centimetres off (tests/test_dense_loop_ref.py measures each):

1. after every step pose k, X and the aligner's result equal tests/dense_loop_ref.py byte for byte, and so does every volume; the poses
   meet the TRUE trajectory within the bounds of tests/test_dense_loop_ref.py; the same sequence gives the same bytes at positions 0
   and 2; the frame that cannot be aligned leaves its sequence's pose and volume untouched while the other two take their step
2. the tracked volumes through ops.TsdfMeshBatch and ops.TsdfRaycastBatch at the true last poses: equal to the restatements, and the
   device's own vertices, normals and depths meet the scene
3. mask=True and a batch of one: the bytes of sequence 1 of the batch of three, and the mask of every step

Every call is a plain launch on the context's stream; the empty frame is input the aligner's rule defines (no sample is matched)."""
import hashlib

import numpy as np
import pytest

import dense_loop_cases as cases
import dense_loop_ref as loop
from dense_align_rig import result_bytes
from srrg2_proslam_amd import ops
from test_dense_loop_ref import STEPS, check_map, check_poses, check_view

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = ("A", "B", "A")
_runs = {}


def digest(volume):
    return hashlib.sha256(volume.tobytes()).hexdigest()


def device_run(hip_ctx, depth_type, names, mask=False):
    """the tracker over the sequences `names`, read after every step -> dict(tracker, steps: steps[k][b] = dict(pose, X, result, mask,
    volume: the sha256 of sequence b's volume after frame k))"""
    import torch
    B = len(names)
    vb = ops.TsdfVolumeBatch(B, *cases.DIMS, 1, cases.ROWS, cases.COLS)
    vb.origin.copy_(torch.tensor([cases.ORIGIN] * B, dtype=torch.float32))
    tracker = ops.DenseTrackerBatch(hip_ctx, vb, cases.FRAMES, cases.CAMERA, depth_type, cases.SCALE[depth_type],
                                    tsdf=dict(voxel_size=cases.VS, truncation=cases.TRUNCATION), raycast=dict(step=cases.VS), mask=mask)
    pose0 = np.stack([cases.true_poses(name)[0].astype(F).reshape(16) for name in names])
    tracker.pose[:, 0].copy_(torch.from_numpy(pose0))
    frames = torch.from_numpy(np.stack([np.array(cases.frames(name, depth_type)) for name in names])).cuda()

    def read(k, X=None):
        hip_ctx.synchronize()
        pose, volume = tracker.pose[:, k].cpu().numpy().reshape(B, 4, 4), vb.volume.cpu().numpy()
        if k == 0:
            return [dict(pose=pose[b], volume=digest(volume[b])) for b in range(B)]
        assert X.data_ptr() == tracker.aligner.X.data_ptr()
        X, results = X.cpu().numpy().reshape(B, 4, 4), tracker.aligner.results()
        classes = tracker.aligner.mask_of(1).cpu().numpy() if mask else [None] * B
        return [dict(pose=pose[b], X=X[b], result=results[b], mask=classes[b], volume=digest(volume[b])) for b in range(B)]

    tracker.start(frames[:, 0])
    steps = [read(0)]
    for k in range(1, cases.FRAMES):
        steps.append(read(k, tracker.step(k, frames[:, k])))
    return dict(tracker=tracker, steps=steps, volume=vb.volume.cpu().numpy())


def batch_of_three(hip_ctx, depth_type):
    """the run tests 1, 2 and 3 share, made once a depth type"""
    if depth_type not in _runs:
        _runs[depth_type] = device_run(hip_ctx, depth_type, NAMES)
    return _runs[depth_type]


def assert_step_equals(got, want, what):
    """one sequence's step on the device against the restatement's, byte for byte"""
    assert got["pose"].tobytes() == want["pose"].tobytes(), (what, "pose", got["pose"], want["pose"])
    assert got["volume"] == want["volume"], (what, "volume")
    if want["X"] is not None:
        assert got["X"].tobytes() == want["X"].tobytes(), (what, "X", got["X"], want["X"])
        assert got["result"].tobytes() == result_bytes(want["result"]), (what, "result", got["result"], want["result"])


# ---- 1. the loop -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth_type", cases.DEPTH_TYPES)
def test_tracker_follows_the_true_trajectory(hip_ctx, depth_type):
    run = batch_of_three(hip_ctx, depth_type)
    steps = run["steps"]
    # the truth first: this does not depend on the restatement
    for b, name in enumerate(NAMES):
        check_poses(name, [steps[k][b]["pose"] for k in range(cases.FRAMES)], "device %s sequence %d" % (depth_type, b))
    # the restatement, step by step
    for b, name in enumerate(NAMES):
        want, volume = loop.tracked(name, depth_type)
        for k in range(cases.FRAMES):
            assert_step_equals(steps[k][b], want[k], (depth_type, name, b, k))
        assert run["volume"][b].tobytes() == volume.tobytes(), (depth_type, name, b)
    # the same sequence at positions 0 and 2
    for k in range(cases.FRAMES):
        for field in steps[k][0]:
            a, c = steps[k][0][field], steps[k][2][field]
            assert (a == c) if field == "volume" else (a is None and c is None) or a.tobytes() == c.tobytes(), (k, field)
    assert run["volume"][0].tobytes() == run["volume"][2].tobytes() != run["volume"][1].tobytes()
    # the frame that cannot be aligned: sequence 1 stays while 0 and 2 take their step in the same launches
    stay, moved = steps[3][1], steps[3][0]
    assert (int(stay["result"]["status"]), int(stay["result"]["num_inliers"]), int(stay["result"]["steps_taken"])) == (0, 0, 0)
    assert stay["pose"].tobytes() == steps[2][1]["pose"].tobytes() and stay["volume"] == steps[2][1]["volume"]
    assert stay["X"].tobytes() == np.eye(4, dtype=F).tobytes()
    assert int(moved["result"]["status"]) == 1 and int(moved["result"]["steps_taken"]) == STEPS
    assert moved["pose"].tobytes() != steps[2][0]["pose"].tobytes() and moved["volume"] != steps[2][0]["volume"]


# ---- 2. the map ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth_type", cases.DEPTH_TYPES)
def test_the_tracked_volumes_mesh_onto_the_scene(hip_ctx, depth_type):
    import torch
    run = batch_of_three(hip_ctx, depth_type)
    tracker = run["tracker"]
    vb = tracker.volumes
    assert vb.volume.cpu().numpy().tobytes() == run["volume"].tobytes()           # as the loop left them
    mb = ops.TsdfMeshBatch(vb, loop.MESH_STRIDE, loop.MESH_STRIDE)
    mb.run(hip_ctx, tracker.tsdf_params)
    last = np.stack([cases.true_poses(name)[-1].astype(F).reshape(1, 16) for name in NAMES])
    rb = ops.TsdfRaycastBatch(hip_ctx, vb, 1, cases.ROWS, cases.COLS)
    rb.run(tracker.raycast_params, torch.from_numpy(last).cuda())
    hip_ctx.synchronize()
    got = {k: getattr(mb, k).cpu().numpy() for k in ("vertex", "normal", "quad", "cube", "edge", "n_vertices", "n_vertices_total",
                                                     "n_quads", "n_quads_total", "status")}
    view = {k: getattr(rb, k).cpu().numpy() for k in ("depth", "normal", "n_hit", "n_skipped", "status")}
    for b, name in enumerate(NAMES):
        what = "device %s sequence %d (%s)" % (depth_type, b, name)
        want = loop.mesh_of(name, depth_type)
        for k in ("n_vertices", "n_vertices_total", "n_quads", "n_quads_total", "status"):
            assert int(got[k][b]) == want[k], (what, k)
        for k in ("vertex", "normal", "quad", "cube", "edge"):
            assert got[k][b].tobytes() == want[k].tobytes(), (what, k)
        n = int(got["n_vertices"][b])
        assert int(got["status"][b]) == 0 and int(got["n_quads"][b]) > 5000
        check_map(got["vertex"][b, :n], got["normal"][b, :n], what)
        seen = loop.view_of(name, depth_type)
        assert (int(view["status"][b]), int(view["n_skipped"][b]), int(view["n_hit"][b, 0])) == (0, 0, int(seen["n_hit"][0])), what
        assert view["depth"][b, 0].tobytes() == seen["depth"][0].tobytes(), what
        assert view["normal"][b, 0].tobytes() == seen["normal"][0].tobytes(), what
        check_view(name, view["depth"][b, 0], what)


# ---- 3. a mask and a batch of one ------------------------------------------------------------------------------------------------------
def test_a_tracker_with_a_mask_and_one_sequence(hip_ctx):
    three = batch_of_three(hip_ctx, "u16")["steps"]
    one = device_run(hip_ctx, "u16", ("B",), mask=True)
    want, volume = loop.tracked("B", "u16")
    for k in range(cases.FRAMES):
        got = one["steps"][k][0]
        for field in ("pose", "X", "result"):
            if field in three[k][1]:
                assert got[field].tobytes() == three[k][1][field].tobytes(), (k, field)
        assert got["volume"] == three[k][1]["volume"], k
        if k:
            assert got["mask"].shape == want[k]["mask"].shape == (cases.ROWS * cases.COLS,)
            assert (got["mask"] == want[k]["mask"]).all(), (k, np.flatnonzero(got["mask"] != want[k]["mask"])[:4].tolist())
    assert not one["steps"][3][0]["mask"].any() and (one["steps"][4][0]["mask"] == 1).sum() > 2500
    assert one["volume"][0].tobytes() == volume.tobytes()
