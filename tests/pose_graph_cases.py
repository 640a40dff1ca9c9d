"""Graphs the pose-graph tests share: seeded synthetic ones for every path of the kernel, and one cut from KITTI-00 ground truth.

A case is a dict(name, poses [n, 16] float64 (the initial guess), fixed [n] uint8, src / dst [E] int32, Z [E, 16] float32, omega
[E, 36] float32 or None, truth [n, 16] float64).  Built once per process (cases(), kitti_case()) and never modified by a test.
"""
import functools
import os

import numpy as np

import pose_graph_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Largest difference between pose_graph_ref.optimize (the kernel's operation order) and pose_graph_ref.optimize_dense (dense LU,
# matrix-form Jacobians) over every case below, criterion off, 5 iterations, damping 0: measured on the CPU by
# tests/test_pose_graph_ref.py::test_restatement_against_dense (it prints both figures).  The two differ in operation order only;
# the test asserts 10 x these.
MEASURED_MAX_DT = 1.9e-4  # metres (kitti114; the synthetic cases stay below 5e-7)
MEASURED_MAX_DQ = 2.8e-7  # quaternion units (kitti114; the synthetic cases stay below 3e-8)


def _rand_pose(rng, t_sigma, q_sigma):
    v = np.concatenate([rng.normal(0, t_sigma, 3), rng.normal(0, q_sigma, 3)])
    return ref.tnq2t(v)


def _graph(name, rng, n, closures=(), fixed=(0,), extra=(), omega_random=False, noise=(0.05, 0.01)):
    """a random walk of n poses, odometry edges i -> i + 1, `closures` (from, to) and `extra` edges; measurements = truth relative
    pose times noise, guess = the chain of noisy odometry"""
    truth = np.zeros((n, 16))
    truth[0] = _rand_pose(rng, 2.0, 0.3)
    for i in range(1, n):
        step = ref.tnq2t(np.concatenate([[1.0, 0.0, 0.0] + rng.normal(0, 0.2, 3), rng.normal(0, 0.08, 3)]))
        truth[i] = ref.se3_mul(truth[i - 1], step)
    edges = [(i, i + 1) for i in range(n - 1)] + list(closures) + list(extra)
    src = np.array([e[0] for e in edges], np.int32).reshape(-1)
    dst = np.array([e[1] for e in edges], np.int32).reshape(-1)
    Zd = np.zeros((len(edges), 16))
    for k, (a, b) in enumerate(edges):
        rel = ref.se3_mul(ref.se3_inverse(truth[a]), truth[b])
        Zd[k] = ref.se3_mul(rel, _rand_pose(rng, *noise))
    Z = Zd.astype(np.float32)
    # the guess is a product of float64 isometries: rotations rounded to float32 are off SO(3) by 6e-8 each, a chain of them by more,
    # and the optimiser keeps whatever its input rotations are (X <- X exp(dx))
    poses = truth.copy()
    for i in range(1, n):
        poses[i] = ref.se3_mul(poses[i - 1], Zd[i - 1])
    fx = np.zeros(n, np.uint8)
    fx[list(fixed)] = 1
    omega = None
    if omega_random:
        omega = np.zeros((len(edges), 36), np.float32)
        for k in range(len(edges)):
            A = rng.normal(0, 1, (6, 6))
            omega[k] = (A @ A.T + 6 * np.eye(6)).astype(np.float32).reshape(-1)
            omega[k] = (0.5 * (omega[k].reshape(6, 6) + omega[k].reshape(6, 6).T)).reshape(-1)
    return dict(name=name, poses=poses, fixed=fx, src=src, dst=dst, Z=Z, omega=omega, truth=truth)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261017)
    out = [
        _graph("n1", rng, 1),
        _graph("n2_one_edge", rng, 2),
        _graph("chain3", rng, 3),
        _graph("ring8", rng, 8, closures=[(7, 0)]),
        _graph("closure_spans_all", rng, 12, closures=[(0, 11)]),
        _graph("two_closures_one_row", rng, 14, closures=[(2, 12), (5, 12)]),
        _graph("closure_from_above", rng, 10, closures=[(9, 3)]),
        _graph("duplicated_edge", rng, 6, closures=[(1, 5)], extra=[(2, 3), (1, 5)]),
        _graph("fixed_not_first", rng, 9, closures=[(1, 8)], fixed=(4,)),
        _graph("two_fixed", rng, 9, closures=[(0, 7)], fixed=(0, 8)),
        _graph("n65", rng, 65, closures=[(0, 64), (10, 40)], noise=(0.02, 0.004)),
        _graph("n130", rng, 130, closures=[(1, 129), (30, 100), (64, 128)], noise=(0.02, 0.004)),
        _graph("omega", rng, 10, closures=[(2, 9), (8, 1)], omega_random=True),
    ]
    return tuple(out)


MIXED_BATCH = ("ring8", "n65", "chain3", "omega", "ring8")  # five graphs of different sizes in one launch; ring8 at slots 0 and 4


def case(name):
    return next(c for c in cases() if c["name"] == name)


def _rows_to_16(rows12):
    T = np.zeros((len(rows12), 16))
    T[:, :12] = rows12
    T[:, 15] = 1.0
    return T


@functools.lru_cache(maxsize=None)
def kitti_case(consistent=False, z_dtype=np.float32, step=40):
    """every 40th pose of KITTI-00 (`city`): 114 nodes, odometry = ground-truth relative pose times a seeded perturbation (sigma
    0.02 m, 0.002 quaternion units), a closure from node j to its nearest earlier node when that is within 6 m and at least 15
    nodes older.  consistent=True: every measurement is exactly the ground-truth relative pose (the recovery test), the guess stays
    the perturbed chain.  step: every step-th pose instead (tools/bench_pose_graph.py uses 10: 455 nodes), closures as many nodes
    older as 600 frames are."""
    gt = _rows_to_16(np.load(os.path.join(GOLDEN, "ref_kitti_gt.npz"))["city"][::step].astype(np.float64))
    n = len(gt)
    rng = np.random.default_rng(40)
    age = 600 // step
    edges = [(i, i + 1) for i in range(n - 1)]
    pos = gt[:, [3, 7, 11]]
    for j in range(n):
        if j >= age:
            d = np.linalg.norm(pos[: j - age + 1] - pos[j], axis=1)
            i = int(np.argmin(d))
            if d[i] <= 6.0:
                edges.append((j, i))
    src, dst = np.array([e[0] for e in edges], np.int32), np.array([e[1] for e in edges], np.int32)
    # the stored rows are float32 and not exactly orthonormal: relative poses are taken between their projections onto SE(3)
    # (through the unit quaternion), so that they are consistent with each other around every loop; `truth` stays the stored rows
    G = ref.tnq2t(ref.t2tnq(gt)[0])
    rel = ref.se3_mul(ref.se3_inverse(G[src]), G[dst])
    noisy = rel.copy()
    for k in range(n - 1):
        noisy[k] = ref.se3_mul(rel[k], _rand_pose(rng, 0.02, 0.002))
    poses = G.copy()
    for i in range(1, n):
        poses[i] = ref.se3_mul(poses[i - 1], noisy[i - 1])  # (float64 isometries: see _graph)
    Z = (rel if consistent else noisy).astype(z_dtype)
    fx = np.zeros(n, np.uint8)
    fx[0] = 1
    return dict(name="kitti%d%s" % (n, "_consistent" if consistent else ""), poses=poses, fixed=fx, src=src, dst=dst, Z=Z, omega=None, truth=gt)


def pose_difference(Xa, Xb):
    """(max |dt|, max |dq|) between two sets of poses [n, 16]"""
    D = ref.se3_mul(ref.se3_inverse(np.asarray(Xa, np.float64).reshape(-1, 16)), np.asarray(Xb, np.float64).reshape(-1, 16))
    v, _ = ref.t2tnq(D)
    return float(np.abs(v[:, :3]).max()), float(np.abs(v[:, 3:]).max())
