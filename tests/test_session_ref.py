"""The local-map manager's rule on the CPU (tests/session_ref.py, the restatement the GPU suite compares bytes with): its float32
criterion against the float64 schedule of tools/bench_tracking.py along all of KITTI-00, the graph and trajectory it builds, the
statuses, and the threshold edges."""
import numpy as np
import pytest

import session_cases as sc
import session_ref as ref

F = np.float32


@pytest.fixture(scope="module")
def gt():
    return sc.kitti00()


@pytest.fixture(scope="module")
def kitti_walk(gt):
    return sc.follow_ground_truth(gt, *sc.SHIPPED["kitti"], node_stride=448)


@pytest.mark.parametrize("name", sorted(sc.SHIPPED))
def test_float32_rule_reproduces_the_float64_schedule_on_kitti00(gt, name):
    """all 4541 poses; the closest threshold margin on the path is 6e-6 relative, a hundred float32 roundings"""
    d, a = sc.SHIPPED[name]
    w, splits = sc.follow_ground_truth(gt, d, a, node_stride=sc.MAPS_ON_KITTI00[name] + 1)
    assert splits == sorted(sc.split_schedule(gt, d, a))
    assert len(splits) + 1 == sc.MAPS_ON_KITTI00[name] == int(w.n_nodes[0]) == int(w.n_edges[0]) + 1
    if name == "kitti":
        assert splits[:3] == [12, 24, 35]


def test_kitti_graph_and_trajectory_against_ground_truth(gt, kitti_walk):
    w, splits = kitti_walk
    n = int(w.n_nodes[0])
    assert (n, int(w.n_edges[0])) == (443, 442)
    assert np.array_equal(w.src[0, :442], np.arange(442)) and np.array_equal(w.dst[0, :442], np.arange(1, 443))
    assert w.fixed[0, 0] == 1 and not w.fixed[0, 1:n].any()
    assert np.array_equal(w.omega[0, :442], np.tile(np.eye(6, dtype=F), (442, 1, 1)))  # every split by viewpoint: information 1
    frames = [0] + splits
    node_dt = float(np.max(np.linalg.norm(w.X[0, :n, :3, 3] - gt[frames, :3, 3], axis=1)))
    un = ref.unroll(w)[0]
    traj_dt = float(np.max(np.linalg.norm(un[:, :3, 3].astype(np.float64) - gt[:, :3, 3], axis=1)))
    exact_nodes, exact_un = sc.follow_ground_truth(gt, *sc.SHIPPED["kitti"], node_stride=0, exact=True)
    exact = max(float(np.max(np.abs(exact_nodes - gt[frames]))), float(np.max(np.abs(exact_un - gt))))
    print("largest node |dt| %.4g m, unrolled |dt| %.4g m; float64 restatement against ground truth %.3g" % (node_dt, traj_dt, exact))
    assert exact < 1e-9
    assert node_dt <= 10 * sc.MEASURED_NODE_DT and traj_dt <= 10 * sc.MEASURED_TRAJECTORY_DT
    # the log: every frame in the node of its map, a split frame still in the old one
    node_of_frame = np.searchsorted(np.array(splits), np.arange(len(gt)), side="left")
    assert np.array_equal(w.frame_node[0], node_of_frame)


def test_threshold_edges():
    d2, cos_a = ref.thresholds(10, 0.25)
    assert d2 == F(100) and cos_a == F(np.cos(np.float64(F(0.25))))
    P = np.eye(4, dtype=F)
    P[2, 3] = F(10)
    assert not ref.criterion(P, d2, cos_a)[0]                      # t2 == d2
    P[2, 3] = np.nextafter(F(10), F(11))
    assert ref.criterion(P, d2, cos_a)[0]                          # one ulp beyond
    # c == cos_a does not split, the next c below it does
    angle, A, B = sc.cosine_edge(0.25)
    assert 0.25 <= angle < 0.2500002
    cos_e = ref.thresholds(10, angle)[1]
    hit, _, c = ref.criterion(A, d2, cos_e)
    assert c == cos_e and not hit
    hit, _, c = ref.criterion(B, d2, cos_e)
    assert c < cos_e and hit
    # icl's 3 rad: a turn by 2.9 rad does not split, the distance does; an angle >= pi never splits by rotation
    d2i, ci = ref.thresholds(5, 3)
    turn = sc.rotation([0, 1, 0], 2.9).astype(F)
    assert not ref.criterion(turn, d2i, ci)[0]
    assert ref.criterion(sc.rotation([0, 1, 0], 3.05).astype(F), d2i, ci)[0]
    assert ref.thresholds(5, np.pi)[1] == F(-np.inf) and ref.thresholds(5, 4.0)[1] == F(-np.inf)
    half = sc.rotation([0, 1, 0], np.pi).astype(F)
    assert not ref.criterion(half, *ref.thresholds(5, np.pi))[0]


def test_lost_frames_split_with_the_lost_information_and_keep_the_prediction():
    w = ref.World(1, 8, 4, 4, 4)
    one, zero = np.ones(1, np.int32), np.zeros(1, np.int32)
    step = sc.translation([0, 0, 1.0]).astype(F)
    X = np.linalg.inv(step)[None].astype(F)  # pose = prediction * X^-1: one metre past the prediction
    ref.step(w, 10, 0.25, X, one, zero, zero)
    ref.step(w, 10, 0.25, X, one, zero, zero)
    pred = w.prediction[0].copy()
    garbage = sc.translation([50, 0, 0])[None].astype(F)
    ref.step(w, 10, 0.25, garbage, zero, zero, zero)  # status 0: lost
    assert w.reason[0] == ref.SPLIT_LOST and w.n_nodes[0] == 2
    assert np.array_equal(w.Z[0, 0], pred) and np.array_equal(w.frame_pose[0, 2], pred)
    assert np.array_equal(w.omega[0, 0], np.eye(6, dtype=F) * F(0.1))
    assert np.array_equal(w.pose[0], np.eye(4, dtype=F)) and w.frame[0] == 0 and w.slot[0] == 1 and w.n_corr_merge[0] == 0
    ref.step(w, 10, 0.25, X, one, -np.ones(1, np.int32), zero)  # a negative warnings word: lost again
    assert w.reason[0] == ref.SPLIT_LOST and w.n_nodes[0] == 3


def test_statuses():
    one, zero = np.ones(1, np.int32), np.zeros(1, np.int32)
    far = np.linalg.inv(sc.translation([0, 0, 11.0]))[None].astype(F)
    w = ref.World(1, 3, 4, 2, 2)
    for _ in range(2):
        ref.step(w, 10, 0.25, far, one, zero, 7 * one)
    assert w.status[0] == ref.OK and w.reason[0] == ref.SPLIT_VIEWPOINT and w.n_nodes[0] == 2
    ref.step(w, 10, 0.25, far, one, zero, 7 * one)  # wants node 2 of node_stride 2: refused, the map goes on
    assert w.status[0] == ref.ERR_CAPACITY and w.reason[0] == ref.NO_SPLIT and w.n_nodes[0] == 2
    assert w.frame[0] == 1 and w.slot[0] == 2 and w.n_corr_merge[0] == 7
    before = w.frame_pose.copy()
    ref.step(w, 100, 0.25, far, one, zero, zero)  # frame 3 of frame_stride 3: the step runs, the log row is skipped
    assert w.status[0] == ref.ERR_CAPACITY and w.n_frames[0] == 4 and np.array_equal(w.frame_pose, before)
    w.slot[0] = -1
    pose = w.pose.copy()
    ref.step(w, 100, 0.25, far, one, zero, zero)
    assert w.status[0] == ref.ERR_RANGE and w.n_frames[0] == 4 and np.array_equal(w.pose, pose)
