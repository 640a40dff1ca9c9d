"""Numpy restatement of the local-map manager (include/proslam_hip.h, prs_session_step_batch / prs_session_unroll_batch), in the
kernels' operation order.  Float32 SE(3) arithmetic goes through the CPU oracle's se3_mul, se3_inverse and motion_predict (the
functions the device's pose_compose and motion_predict kernels are tested against); the criterion is numpy float32 scalars, one
rounding per operation; the float64 node product is explicit loops in the order of se3_mul.

The state of B sequences is a `World`: plain arrays in the device layout, so that a test compares array with array."""
import numpy as np

from oracle import binding as ob

OK, ERR_CAPACITY, ERR_RANGE = 0, -2, -4
NO_SPLIT, SPLIT_VIEWPOINT, SPLIT_LOST = 0, 1, 2
F = np.float32


def thresholds(distance, angle):
    """(d2, cos_a) as the launcher forms them: the square in float32, the cosine in float64 of the float32 angle, rounded once"""
    d = F(distance)
    a = np.float64(F(angle))
    return F(d * d), (F(-np.inf) if a >= np.pi else F(np.cos(a)))


def criterion(pose, d2, cos_a):
    p = np.asarray(pose, F).reshape(4, 4)
    t2 = F(F(F(p[0, 3] * p[0, 3]) + F(p[1, 3] * p[1, 3])) + F(p[2, 3] * p[2, 3]))
    c = F(F(F(F(p[0, 0] + p[1, 1]) + p[2, 2]) - F(1.0)) * F(0.5))
    return bool(t2 > d2 or c < cos_a), t2, c


def se3_mul_f64(A, B):
    """the expressions of prs::se3_mul in float64"""
    A, B = np.asarray(A, np.float64).reshape(4, 4), np.asarray(B, np.float64).reshape(4, 4)
    C = np.zeros((4, 4), np.float64)
    for i in range(3):
        for j in range(3):
            C[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
        C[i, 3] = ((A[i, 0] * B[0, 3] + A[i, 1] * B[1, 3]) + A[i, 2] * B[2, 3]) + A[i, 3]
    C[3, 3] = 1.0
    return C


class World:
    """B sessions with their maps, graphs and the optional hand-over slots, as the device holds them"""

    def __init__(self, batch, frame_stride, capacity, node_stride, edge_stride, handover_stride=0, with_omega=True):
        B = batch
        self.batch, self.frame_stride, self.capacity = B, frame_stride, capacity
        self.node_stride, self.edge_stride, self.handover_stride = node_stride, edge_stride, handover_stride
        eye = np.tile(np.eye(4, dtype=F), (B, 1, 1))
        self.pose, self.prev, self.prediction = eye.copy(), eye.copy(), eye.copy()
        self.slot, self.cur_node, self.n_frames = (np.zeros(B, np.int32) for _ in range(3))
        self.frame_node = np.zeros((B, frame_stride), np.int32)
        self.frame_pose = np.zeros((B, frame_stride, 4, 4), F)
        self.status, self.reason = np.zeros(B, np.int32), np.zeros(B, np.int32)
        # the map and the merger's per-frame inputs
        self.coords = np.zeros((B, capacity, 4), F)
        self.desc = np.zeros((B, capacity, 32), np.uint8)
        self.n_points = np.zeros(B, np.int32)
        self.n_meas = np.zeros((B, capacity), np.uint32)
        self.frame, self.n_corr_merge = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.measurement_in_world, self.measurement_in_scene = eye.copy(), eye.copy()
        # the graphs
        self.X = np.tile(np.eye(4), (B, node_stride, 1, 1))
        self.fixed = np.zeros((B, node_stride), np.uint8)
        self.n_nodes, self.n_edges = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.src, self.dst = np.zeros((B, edge_stride), np.int32), np.zeros((B, edge_stride), np.int32)
        self.Z = np.zeros((B, edge_stride, 4, 4), F)
        self.omega = np.zeros((B, edge_stride, 6, 6), F) if with_omega else None
        # the hand-over
        hs = max(handover_stride, 1)
        self.handover = handover_stride > 0
        self.handover_desc = np.zeros((B, hs, 32), np.uint8)
        self.handover_xyz = np.zeros((B, hs, 4), F)
        self.handover_n_query = np.zeros(B, np.int32)
        self.handover_graph_id = np.zeros(B, np.int64)
        self.graph_id_base = None
        self.reset()

    def reset(self):
        eye = np.eye(4, dtype=F)
        self.pose[:], self.prev[:], self.prediction[:] = eye, eye, eye
        for a in (self.slot, self.cur_node, self.n_frames, self.status, self.reason, self.n_corr_merge):
            a[:] = 0
        self.X[:, 0] = np.eye(4)
        self.fixed[:, 0] = 1
        self.n_nodes[:] = 1
        self.n_edges[:] = 0


def step(w, distance, angle, X, align_status, align_warnings, n_corr, split_information=1.0, lost_information=0.1):
    """one frame of every sequence of `w`, in place.  X [B, 4, 4] float32, align_status / align_warnings / n_corr [B]"""
    d2, cos_a = thresholds(distance, angle)
    I4 = np.eye(4, dtype=F)
    for b in range(w.batch):
        k, slot, cur = int(w.n_frames[b]), int(w.slot[b]), int(w.cur_node[b])
        nn, ne, npts = int(w.n_nodes[b]), int(w.n_edges[b]), int(w.n_points[b])
        bad = (k < 0 or slot < 0 or cur < 0 or nn < 0 or ne < 0 or npts < 0 or cur >= nn or nn > w.node_stride or ne > w.edge_stride
               or npts > w.capacity)
        if bad:
            w.status[b], w.reason[b] = ERR_RANGE, NO_SPLIT
            if w.handover:
                w.handover_n_query[b] = 0
            continue
        status, want = OK, NO_SPLIT
        if k == 0:
            pose_new, prev_new = I4.copy(), I4.copy()
        else:
            pred = w.prediction[b].copy()
            prev_new = w.pose[b].copy()
            lost = int(align_status[b]) != 1 or int(align_warnings[b]) < 0
            pose_new = pred if lost else ob.se3_mul(pred, ob.se3_inverse(np.asarray(X[b], F).reshape(4, 4)))
            want = SPLIT_LOST if lost else (SPLIT_VIEWPOINT if criterion(pose_new, d2, cos_a)[0] else NO_SPLIT)
        if k < w.frame_stride:
            w.frame_node[b, k], w.frame_pose[b, k] = cur, pose_new
        else:
            status = ERR_CAPACITY
        if want != NO_SPLIT and (nn >= w.node_stride or ne >= w.edge_stride):
            status, want = ERR_CAPACITY, NO_SPLIT
        n_query = 0
        if want != NO_SPLIT:
            w.X[b, nn] = se3_mul_f64(w.X[b, cur], pose_new.astype(np.float64))
            w.fixed[b, nn] = 0
            w.src[b, ne], w.dst[b, ne], w.Z[b, ne] = cur, nn, pose_new
            if w.omega is not None:
                w.omega[b, ne] = np.eye(6, dtype=F) * F(lost_information if want == SPLIT_LOST else split_information)
            w.n_nodes[b], w.n_edges[b], w.cur_node[b] = nn + 1, ne + 1, nn
            prev_out = ob.se3_mul(ob.se3_inverse(pose_new), prev_new)
            pose_out = I4.copy()
            frame, n_corr_merge = 0, 0
            if w.handover:
                w.handover_xyz[b, :npts], w.handover_desc[b, :npts] = w.coords[b, :npts], w.desc[b, :npts]
                w.handover_graph_id[b] = (int(w.graph_id_base[b]) if w.graph_id_base is not None else 0) + cur
            n_query = npts
            w.n_points[b] = 0
            w.n_meas[b, :] = 0
        else:
            pose_out, prev_out = pose_new, prev_new
            frame, n_corr_merge = (0, 0) if k == 0 else (slot, int(n_corr[b]))
        w.pose[b], w.prev[b] = pose_out, prev_out
        w.prediction[b] = ob.motion_predict(prev_out, pose_out)
        w.measurement_in_world[b], w.measurement_in_scene[b] = pose_out, pose_out
        w.frame[b], w.n_corr_merge[b], w.slot[b], w.n_frames[b] = frame, n_corr_merge, frame + 1, k + 1
        w.status[b], w.reason[b] = status, want
        if w.handover:
            w.handover_n_query[b] = n_query


def unroll(w, out=None):
    """out[b][k] = (float) X[b][frame_node[b][k]] * frame_pose[b][k]; rows past n_frames[b] keep what `out` held"""
    out = np.zeros((w.batch, w.frame_stride, 4, 4), F) if out is None else out
    for b in range(w.batch):
        for k in range(min(max(int(w.n_frames[b]), 0), w.frame_stride)):
            node = int(w.frame_node[b, k])
            if 0 <= node < w.node_stride:
                out[b, k] = ob.se3_mul(w.X[b, node].astype(F), w.frame_pose[b, k])
    return out
