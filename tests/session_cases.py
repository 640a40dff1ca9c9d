"""Inputs shared by the local-map manager's tests (tests/session_ref.py is the restatement they are compared with)."""
import os
import sys

import numpy as np

import session_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
F = np.float32

# (distance, angle) of the shipped configurations (tests/golden/ref_conf_split.json) and, along all 4541 KITTI-00 poses, the number
# of local maps tools/bench_tracking.py's float64 split_schedule gives for them (443 for kitti: frames 12, 24, 35 split first)
SHIPPED = {"kitti": (10, 0.25), "icl": (5, 3), "euroc": (1, 0.5), "tum": (1, 0.25)}
MAPS_ON_KITTI00 = {"kitti": 443, "icl": 686, "euroc": 2741, "tum": 2741}

# test_session_ref.py::test_kitti_graph_and_trajectory_against_ground_truth prints these: the largest distance of a node of the
# float32-measured graph, and of an unrolled pose, from the float64 ground truth along the 3.7 km of KITTI-00 (kitti settings).  The
# float64 restatement of the same walk (follow_ground_truth(..., exact=True)) stays below 1e-9 m, so the figures are what rounding
# the 442 edge measurements and the logged poses to float32 costs.  The tests assert 10 x these (the convention of
# pose_graph_cases.py).
MEASURED_NODE_DT = 5.4e-4        # metres (measured 5.303e-4)
MEASURED_TRAJECTORY_DT = 5.3e-4  # metres (measured 5.287e-4)


def kitti00(n=None):
    """camera k in the first camera's frame, float64 [n, 4, 4]"""
    gt = np.load(os.path.join(GOLDEN, "ref_kitti_gt.npz"))["city"][:n].astype(np.float64)
    T = np.tile(np.eye(4), (len(gt), 1, 1))
    T[:, :3, :4] = gt.reshape(-1, 3, 4)
    return np.linalg.inv(T[0]) @ T


def split_schedule(poses, distance, angle):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_tracking
    return bench_tracking.split_schedule(poses, distance, angle)


def follow_ground_truth(poses, distance, angle, node_stride, exact=False):
    """one session that follows `poses` with a perfect aligner: at frame k the alignment X is the one that makes prediction * X^-1
    the true pose in the current local map, formed in float64 and rounded once to float32 -> (World, frames that split).
    exact=True: the same walk with every pose kept in float64 (what the rule gives without float32 rounding): -> (node poses, unrolled)"""
    n = len(poses)
    if exact:
        origin, nodes, out = np.eye(4), [np.eye(4)], []
        d2, cos_a = float(distance) ** 2, (np.cos(float(angle)) if angle < np.pi else -np.inf)
        for k in range(n):
            local = np.linalg.inv(origin) @ poses[k]
            out.append(origin @ local)
            t2 = float(local[:3, 3] @ local[:3, 3])
            if k > 0 and (t2 > d2 or (np.trace(local[:3, :3]) - 1.0) * 0.5 < cos_a):
                origin = origin @ local
                nodes.append(origin)
        return np.array(nodes), np.array(out)
    w = ref.World(1, n, 1, node_stride, node_stride)
    splits, origin = [], np.eye(4)
    one, zero = np.ones(1, np.int32), np.zeros(1, np.int32)
    for k in range(n):
        local = np.linalg.inv(origin) @ poses[k]
        X = (np.linalg.inv(local) @ w.prediction[0].astype(np.float64)).astype(F)
        ref.step(w, distance, angle, X[None], one, zero, zero)
        assert w.status[0] == ref.OK, (k, w.status[0])
        if w.reason[0] != ref.NO_SPLIT:
            splits.append(k)
            origin = poses[k]
    return w, splits


def rotation(axis, angle):
    """float64 4x4 rotation about a unit axis (Rodrigues)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return T


def translation(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def cosine_edge(angle_from=0.25):
    """(angle, A, B): the first float32 angle at or above angle_from whose threshold cos_a = (float) cos(angle) is a value the
    criterion's c = (((r00 + r11) + r22) - 1) * 0.5f can take exactly (the sum near 3 has half the resolution of cos_a, so every
    other threshold cannot be hit), with A = diag(1, 1, r22, 1) giving c == cos_a and B the same with r22 one ulp lower, c < cos_a"""
    angle = F(angle_from)
    for _ in range(64):
        cos_a = ref.thresholds(1, angle)[1]
        r = F(F(F(2) * cos_a) - F(1))
        for _ in range(4):
            r = np.nextafter(r, F(2))
        for _ in range(9):
            A = np.eye(4, dtype=F)
            A[2, 2] = r
            if ref.criterion(A, F(np.inf), cos_a)[2] == cos_a:
                B = A.copy()
                while ref.criterion(B, F(np.inf), cos_a)[2] >= cos_a:
                    B[2, 2] = np.nextafter(B[2, 2], F(-1))
                return angle, A, B
            r = np.nextafter(r, F(-1))
        angle = np.nextafter(angle, F(4))
    raise AssertionError("no reachable threshold near %r" % (angle_from,))
