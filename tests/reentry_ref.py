"""Numpy restatement of map re-entry (include/proslam_hip.h: prs_map_archive, prs_session_step_archive_batch,
prs_session_reenter_batch), in the kernels' operation order.  The step itself is tests/session_ref.py's; the float32 SE(3) arithmetic
goes through the CPU oracle's se3_mul, se3_inverse and motion_predict, the gates are numpy float32 scalars with one rounding per
operation.

The state is plain arrays in the device layout, so that a test compares array with array: `session_ref.World` for the session, the
map's coords / desc / n_meas and the graphs, `LiveMaps` for the statistics arrays the session batch does not carry, `Archive` for
the archive, `Detector` for the loop detector's outputs and `Reentry` for the outputs of the re-entry launch."""
import numpy as np

from oracle import binding as ob

import session_ref as sr

OK, ERR_CAPACITY, ERR_RANGE = sr.OK, sr.ERR_CAPACITY, sr.ERR_RANGE
F = np.float32
MEAS_WORDS, POSE_WORDS = 7, 24
RESULT_WORDS = 52  # prs_point_align_result: H 36, b 6, chi_inliers, chi_total, then 8 int32
R_CHI_INLIERS, R_NUM_INLIERS, R_NUM_CORR, R_STATUS, R_ACCEPTED = 42, 44, 47, 48, 49
ROW_ARRAYS = ("coords", "desc", "state", "covariance", "n_opt", "inlier", "n_meas")


class LiveMaps:
    """the arrays of prs_merge_batch that prs_session_batch does not carry"""

    def __init__(self, batch, capacity, max_measurements=0, max_frames=1):
        self.max_measurements, self.max_frames = max_measurements, max_frames
        self.state = np.zeros((batch, capacity, 4), F)
        self.covariance = np.zeros((batch, capacity, 9), F)
        self.n_opt = np.zeros((batch, capacity), np.uint32)
        self.inlier = np.zeros((batch, capacity), np.uint8)
        self.meas = np.zeros((batch, capacity, max(max_measurements, 1), MEAS_WORDS), np.int32)
        self.poses = np.zeros((batch, max_frames, POSE_WORDS), F)
        self.n_measured = np.zeros(batch, np.int32)


class Archive:
    def __init__(self, batch, capacity, slot_stride, node_stride, max_measurements=0, max_frames=0):
        """max_measurements > 0: the history and the pose table are kept"""
        B, S = batch, slot_stride
        self.batch, self.capacity, self.slot_stride, self.node_stride = B, capacity, S, node_stride
        self.history = max_measurements > 0
        self.max_measurements, self.max_frames = max_measurements, max_frames
        self.coords, self.desc = np.zeros((B, S, capacity, 4), F), np.zeros((B, S, capacity, 32), np.uint8)
        self.state, self.covariance = np.zeros((B, S, capacity, 4), F), np.zeros((B, S, capacity, 9), F)
        self.n_opt, self.inlier = np.zeros((B, S, capacity), np.uint32), np.zeros((B, S, capacity), np.uint8)
        self.n_meas = np.zeros((B, S, capacity), np.uint32)
        self.n_points, self.next_frame = np.zeros((B, S), np.int32), np.zeros((B, S), np.int32)
        self.meas = np.zeros((B, S, capacity, max_measurements, MEAS_WORDS), np.int32) if self.history else None
        self.poses = np.zeros((B, S, max_frames, POSE_WORDS), F) if self.history else None
        self.slot_of_node = np.full((B, node_stride), -1, np.int32)
        self.n_slots, self.status = np.zeros(B, np.int32), np.zeros(B, np.int32)

    def arrays(self):
        names = ROW_ARRAYS + ("n_points", "next_frame", "slot_of_node", "n_slots", "status") + (("meas", "poses") if self.history else ())
        return {n: getattr(self, n) for n in names}


def _live(w, live, name):
    return getattr(w, name) if name in ("coords", "desc", "n_meas") else getattr(live, name)


def step_archive(w, live, arch, distance, angle, X, align_status, align_warnings, n_corr, **information):
    """session_ref.step, and the finished maps go to the archive before they are reset"""
    before = dict(cur=w.cur_node.copy(), slot=w.slot.copy(), n_points=w.n_points.copy(), n_meas=w.n_meas.copy())
    sr.step(w, distance, angle, X, align_status, align_warnings, n_corr, **information)
    for b in range(w.batch):
        arch.status[b] = OK
        if w.reason[b] == sr.NO_SPLIT:
            continue
        cur, n = int(before["cur"][b]), int(before["n_points"][b])
        s = int(arch.slot_of_node[b, cur])
        if s >= arch.slot_stride:
            arch.status[b] = ERR_RANGE
            continue
        if s < 0:
            ns = int(arch.n_slots[b])
            if ns < 0 or ns >= arch.slot_stride:
                arch.status[b] = ERR_CAPACITY
                continue
            s = ns
            arch.n_slots[b], arch.slot_of_node[b, cur] = ns + 1, ns
        arch.n_points[b, s], arch.next_frame[b, s] = n, before["slot"][b]
        for name in ROW_ARRAYS:
            src = before["n_meas"] if name == "n_meas" else _live(w, live, name)
            getattr(arch, name)[b, s, :n] = src[b, :n]
        if arch.history:
            arch.meas[b, s, :n] = live.meas[b, :n]
            arch.poses[b, s] = live.poses[b]


class Detector:
    """the loop detector's outputs the re-entry reads: B sequences of max_candidates slots"""

    def __init__(self, batch, max_candidates, map_stride, corr_stride):
        K = max_candidates
        self.max_candidates, self.map_stride, self.corr_stride = K, map_stride, corr_stride
        self.candidates_flat = np.full((batch, K), -1, np.int32)
        self.result = np.zeros((batch * K, RESULT_WORDS), np.int32)
        self.X = np.tile(np.eye(4, dtype=F), (batch * K, 1, 1))
        self.corr = np.zeros((batch * K, corr_stride, 3), np.int32)
        self.n_corr = np.zeros(batch * K, np.int32)
        self.node_of_map = np.full((batch, map_stride), -1, np.int32)

    def plant(self, b, k, map_index, node, X, num_inliers, num_correspondences, chi_inliers, accepted=1, corr=None):
        """slot k of sequence b holds map `map_index` of the bank (stored for `node`) with the given aligner result"""
        s = b * self.max_candidates + k
        self.candidates_flat[b, k] = b * self.map_stride + map_index if map_index >= 0 else -1
        if map_index >= 0:
            self.node_of_map[b, map_index] = node
        self.X[s] = np.asarray(X, F).reshape(4, 4)
        r = self.result[s]
        r[:] = np.arange(RESULT_WORDS) + 1000 * (k + 1)  # the words the rule does not read travel with the gate
        r[R_NUM_INLIERS], r[R_NUM_CORR], r[R_STATUS], r[R_ACCEPTED] = num_inliers, num_correspondences, 1, accepted
        r[R_CHI_INLIERS: R_CHI_INLIERS + 1] = np.array([chi_inliers], F).view(np.int32)
        if corr is not None:
            c = np.asarray(corr, np.int32).reshape(-1, 3)
            self.corr[s, : len(c)], self.n_corr[s] = c, len(c)


class Reentry:
    def __init__(self, batch, corr_stride, fill=0):
        self.reentered, self.status = np.full(batch, fill, np.int32), np.full(batch, fill, np.int32)
        self.merge_corr = np.full((batch, corr_stride, 3), fill, np.int32)
        self.merge_n_corr = np.full(batch, fill, np.int32)
        self.merge_transform = np.full((batch, 4, 4), fill, F)
        self.scene_in_world = np.full((batch, 4, 4), fill, F)
        self.gate = np.full((batch, RESULT_WORDS), fill, np.int32)

    def arrays(self):
        return {n: getattr(self, n) for n in ("reentered", "status", "merge_corr", "merge_n_corr", "merge_transform", "scene_in_world", "gate")}


def params(max_translation, relocalize_min_inliers, relocalize_min_inliers_ratio, relocalize_max_chi_inliers):
    return dict(max_translation=max_translation, relocalize_min_inliers=relocalize_min_inliers,
                relocalize_min_inliers_ratio=relocalize_min_inliers_ratio, relocalize_max_chi_inliers=relocalize_max_chi_inliers)


def translation2(P):
    P = np.asarray(P, F).reshape(4, 4)
    return F(F(F(P[0, 3] * P[0, 3]) + F(P[1, 3] * P[1, 3])) + F(P[2, 3] * P[2, 3]))


def qualifies(P, det, arch, b, k, f, m, n_nodes, Z):
    """-> (num_inliers, o, pose in o) if candidate slot k of sequence b passes every gate, else None"""
    s = b * det.max_candidates + k
    c = int(det.candidates_flat[b, k])
    mi = c - b * det.map_stride
    r = det.result[s]
    if c < 0 or mi < 0 or mi >= det.map_stride or r[R_ACCEPTED] == 0:
        return None
    o = int(det.node_of_map[b, mi])
    if o < 0 or o >= n_nodes or o == f or o == m or arch.slot_of_node[b, o] < 0:
        return None
    ni, nc = int(r[R_NUM_INLIERS]), int(r[R_NUM_CORR])
    chi = r[R_CHI_INLIERS: R_CHI_INLIERS + 1].view(F)[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        if not ni >= int(P["relocalize_min_inliers"]):
            return None
        if not F(F(ni) / F(nc)) >= F(P["relocalize_min_inliers_ratio"]):
            return None
        if not F(chi / F(ni)) <= F(P["relocalize_max_chi_inliers"]):
            return None
    pose = ob.se3_mul(ob.se3_inverse(det.X[s]), np.asarray(Z, F).reshape(4, 4))
    mt = F(P["max_translation"])
    if not translation2(pose) <= F(mt * mt):
        return None
    return ni, o, pose


def reenter(w, live, arch, det, out, P):
    """the re-entry launch for every sequence of `w`, in place"""
    for b in range(w.batch):
        go, status = False, OK
        if w.reason[b] == sr.SPLIT_VIEWPOINT and w.status[b] == OK:
            nn, ne, cur = int(w.n_nodes[b]), int(w.n_edges[b]), int(w.cur_node[b])
            m = nn - 1
            into = [j for j in range(max(min(ne, w.edge_stride), 0)) if w.dst[b, j] == m]
            if nn < 1 or nn > w.node_stride or ne < 0 or ne > w.edge_stride or cur != m:
                status = ERR_RANGE
            elif len(into) != 1 or not 0 <= w.src[b, into[0]] < m:
                status = ERR_RANGE
            else:
                e = into[0]
                f = int(w.src[b, e])
                best = None
                for k in range(det.max_candidates):
                    q = qualifies(P, det, arch, b, k, f, m, nn, w.Z[b, e])
                    if q is not None and (best is None or q[0] > best[1][0]):
                        best = (k, q)
                if best is not None:
                    k, (_, o, pose) = best
                    s = b * det.max_candidates + k
                    aslot = int(arch.slot_of_node[b, o])
                    n = int(arch.n_points[b, aslot]) if aslot < arch.slot_stride else -1
                    nc = int(det.n_corr[s])
                    if aslot >= arch.slot_stride or n < 0 or n > w.capacity or nc < 0 or nc > det.corr_stride:
                        status = ERR_RANGE
                    else:
                        go = True
        out.status[b], out.reentered[b] = status, 1 if go else 0
        if not go:
            if status == OK:
                out.gate[b, R_ACCEPTED], out.merge_n_corr[b] = 0, 0
            continue
        # graph
        for arr in (w.src, w.dst, w.Z) + ((w.omega,) if w.omega is not None else ()):
            arr[b, e: ne - 1] = arr[b, e + 1: ne].copy()
        w.n_edges[b], w.n_nodes[b], w.cur_node[b] = ne - 1, nn - 1, o
        # session
        prev = ob.se3_mul(pose, w.prev[b])
        w.pose[b], w.prev[b] = pose, prev
        w.prediction[b] = ob.motion_predict(prev, pose)
        w.measurement_in_world[b], w.measurement_in_scene[b] = pose, pose
        # map
        for name in ROW_ARRAYS:
            _live(w, live, name)[b, :n] = getattr(arch, name)[b, aslot, :n]
        w.n_points[b] = n
        if arch.history:
            w.n_meas[b, n:] = 0
            live.meas[b, :n], live.poses[b] = arch.meas[b, aslot, :n], arch.poses[b, aslot]
            frame = int(arch.next_frame[b, aslot])
        else:
            w.n_meas[b, :] = 0
            frame = 0
        w.frame[b], w.slot[b] = frame, frame + 1
        # the two mergers
        w.n_corr_merge[b], live.n_measured[b] = 0, 0
        out.merge_corr[b, :nc], out.merge_n_corr[b] = det.corr[s, :nc], nc
        out.merge_transform[b] = det.X[s]
        out.scene_in_world[b] = w.X[b, o].astype(F)
        out.gate[b] = det.result[s]
        out.gate[b, R_ACCEPTED] = 1
