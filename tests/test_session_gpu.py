"""The local-map manager on the device (ops.SessionBatch: prs_session_step_batch, prs_session_unroll_batch) against its numpy
restatement (tests/session_ref.py).  Every compared array is byte-equal, after every frame."""
import ctypes as C

import numpy as np
import pytest

import session_cases as sc
import session_ref as ref
from srrg2_proslam_amd import _lib, configs, ops, synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32


class Rig:
    """a SessionBatch over small maps, aligner outputs and graphs, and the World that mirrors it"""

    def __init__(self, B, frame_stride, capacity, node_stride, edge_stride, handover_stride=0, with_omega=True):
        self.maps = ops.MapBatch(0, B, capacity, 1, 4, 1, 1)
        self.frames = ops.AlignFrames(0, B, 1, 1)
        self.graphs = ops.PoseGraphBatch(0, B, node_stride, edge_stride, envelope_blocks=4 * node_stride, with_omega=with_omega)
        self.queries = ops.PlaceQueries(0, B, handover_stride, 1) if handover_stride else None
        self.sess = ops.SessionBatch(0, self.maps, self.frames, self.graphs, frame_stride, handover=self.queries)
        self.w = ref.World(B, frame_stride, capacity, node_stride, edge_stride, handover_stride, with_omega)
        self.B = B

    def set_map(self, coords=None, desc=None, n_points=None, n_meas=None):
        """the same map contents on both sides"""
        import torch
        w, m = self.w, self.maps
        for name, value in (("coords", coords), ("desc", desc), ("n_points", n_points), ("n_meas", n_meas)):
            if value is not None:
                getattr(w, name)[...] = value
                t = getattr(m, name)
                src = getattr(w, name)
                t.copy_(torch.from_numpy(src.view(np.int32) if src.dtype == np.uint32 else src).to(t.device))

    def set_handover(self, desc_byte, xyz_value, n_query, graph_id):
        w, q = self.w, self.queries
        w.handover_desc[...], w.handover_xyz[...], w.handover_n_query[...], w.handover_graph_id[...] = desc_byte, xyz_value, n_query, graph_id
        q.desc.fill_(desc_byte)
        q.xyz.fill_(xyz_value)
        q.n_query.fill_(n_query)
        q.graph_id.fill_(graph_id)

    def set_alignment(self, X, status, warnings, n_corr):
        import torch
        f = self.frames
        f.X.copy_(torch.from_numpy(np.ascontiguousarray(X, F).reshape(self.B, 16)).to(f.X.device))
        raw = np.zeros((self.B, C.sizeof(ops.AlignResult)), np.uint8)
        words = raw.view(np.int32)
        words[:, ops.AlignResult.status.offset // 4] = status
        words[:, ops.AlignResult.warnings.offset // 4] = warnings
        f.result.copy_(torch.from_numpy(raw).to(f.result.device))
        f.n_corr.copy_(torch.from_numpy(np.asarray(n_corr, np.int32)).to(f.n_corr.device))

    def step(self, ctx, distance, angle, X, status, warnings, n_corr):
        self.set_alignment(X, status, warnings, n_corr)
        self.sess.step(ctx, ops.session_params(dict(local_map_distance=distance, local_map_angle_distance_radians=angle)))
        ref.step(self.w, distance, angle, X, status, warnings, n_corr)

    def device_arrays(self):
        s, m, g, q = self.sess, self.maps, self.graphs, self.queries
        out = dict(pose=s.pose, prev=s.prev, prediction=s.prediction, slot=s.slot, cur_node=s.cur_node, n_frames=s.n_frames,
                   frame_node=s.frame_node, frame_pose=s.frame_pose, status=s.status, reason=s.reason, n_corr_merge=s.n_corr_merge,
                   n_points=m.n_points, n_meas=m.n_meas, frame=m.frame, measurement_in_world=m.measurement_in_world,
                   measurement_in_scene=m.measurement_in_scene, X=g.X, fixed=g.fixed, n_nodes=g.n_nodes, n_edges=g.n_edges, src=g.src,
                   dst=g.dst, Z=g.Z)
        if g.omega is not None:
            out["omega"] = g.omega
        if q is not None:
            out.update(handover_desc=q.desc, handover_xyz=q.xyz, handover_n_query=q.n_query, handover_graph_id=q.graph_id)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def assert_equal(self, what=""):
        assert self.maps.n_corr is self.sess.n_corr_merge  # the merger reads the session's count
        for name, got in self.device_arrays().items():
            want = getattr(self.w, name)
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (what, name)


def _small(rng, scale_t=2e-3, scale_r=1e-3):
    """a small rigid motion, float64"""
    T = sc.rotation(rng.normal(size=3), rng.normal() * scale_r)
    T[:3, 3] = rng.normal(size=3) * scale_t
    return T


def planted_inputs(n_frames=24, seed=11):
    """X, status, warnings, n_corr per frame for the five planted sequences: 0 translates (0.9 m a frame), 1 turns (0.03 rad a
    frame), 2 stands still, 3 creeps and loses track at frames 3 and 9, 4 races (3 m a frame) into the graph's last node.  After
    the first motion the constant-velocity prediction carries the sequences, the alignments only add small corrections."""
    rng = np.random.default_rng(seed)
    kick = [sc.translation([0, 0, 0.9]), sc.rotation([0.1, 1, 0], 0.03), np.eye(4), sc.translation([0.05, 0, 0]), sc.translation([0, 0.2, 3.0])]
    frames = []
    for k in range(n_frames):
        X = np.zeros((5, 4, 4), F)
        for b in range(5):
            motion = np.eye(4) if b == 2 else ((kick[b] if k == 1 else np.eye(4)) @ _small(rng))
            X[b] = np.linalg.inv(motion).astype(F)  # pose = prediction * X^-1
        status, warnings = np.ones(5, np.int32), np.full(5, 8, np.int32)
        if k == 3:
            status[3] = 0
        if k == 9:
            warnings[3] = -2
        frames.append((X, status, warnings, np.array([30 + k, 40 + k, 50 + k, 60 + k, 70 + k], np.int32)))
    return frames


def _planted_run(hip_ctx, rig, frames, pick=None):
    """pick: run sequence `pick` of the five alone (a rig of one)"""
    rng = np.random.default_rng(5)
    B, cap = rig.B, rig.w.capacity
    sel = (lambda a: a) if pick is None else (lambda a: a[pick: pick + 1])
    rig.set_map(coords=sel(rng.normal(size=(5, cap, 4)).astype(F)), desc=sel(rng.integers(0, 256, (5, cap, 32), dtype=np.uint8)))
    if rig.queries is not None:
        rig.set_handover(0xAB, 7.5, -3, -9)
    log = []
    for k, (X, status, warnings, n_corr) in enumerate(frames):
        # what the merger would have left: some landmarks with measurements
        rig.set_map(n_points=np.full(B, 10 + k, np.int32), n_meas=sel(rng.integers(1, 5, (5, cap)).astype(np.uint32)))
        rig.step(hip_ctx, 10, 0.25, sel(X), sel(status), sel(warnings), sel(n_corr))
        rig.assert_equal("frame %d" % k)
        log.append((rig.w.reason.copy(), rig.w.status.copy()))
    return log


def test_planted_motions(hip_ctx):
    rig = Rig(5, 24, 37, 3, 3, handover_stride=40)
    log = _planted_run(hip_ctx, rig, planted_inputs())
    reason, status = np.array([r for r, _ in log]), np.array([s for _, s in log])
    splits = [list(np.nonzero(reason[:, b])[0]) for b in range(5)]
    assert splits[0] == [12, 23] and list(reason[splits[0], 0]) == [ref.SPLIT_VIEWPOINT] * 2  # crosses 10 m twice
    assert splits[1] == [9, 17] and list(reason[splits[1], 1]) == [ref.SPLIT_VIEWPOINT] * 2  # crosses 0.25 rad twice
    assert splits[2] == [] and not status[:, 2].any()                                      # standstill
    assert splits[3] == [3, 9] and list(reason[splits[3], 3]) == [ref.SPLIT_LOST] * 2
    assert np.array_equal(rig.w.omega[3, :2], np.stack([np.eye(6, dtype=F) * F(0.1)] * 2))
    assert splits[4] == [4, 8] and rig.w.n_nodes[4] == 3                                   # the third split finds no node
    assert list(np.nonzero(status[:, 4])[0]) == list(range(12, 24)) and (status[12:, 4] == ref.ERR_CAPACITY).all()
    assert not status[:, :4].any()
    # the trajectories through the graph, and again after an optimisation with one planted closure in sequence 1
    import torch
    rig.sess.trajectory.fill_(-1.0)
    rig.sess.n_frames[2] = 0
    rig.w.n_frames[2] = 0
    want = ref.unroll(rig.w, np.full((5, 24, 4, 4), -1.0, F))
    got = rig.sess.unroll(hip_ctx).cpu().numpy().reshape(5, 24, 4, 4)
    assert got.tobytes() == want.tobytes() and (got[2] == -1).all() and not (got[1] == -1).any()
    g = rig.graphs
    closure = (np.linalg.inv(rig.w.X[1, 0]) @ rig.w.X[1, 2] @ _small(np.random.default_rng(2), 0.05, 0.01)).astype(F)
    g.src[1, 2], g.dst[1, 2], g.n_edges[1] = 0, 2, 3
    g.Z[1, 2] = torch.from_numpy(closure.reshape(16)).to(g.Z.device)
    g.omega[1, 2] = torch.eye(6, dtype=torch.float32, device=g.omega.device).reshape(36)
    before = g.X.cpu().numpy().copy()
    ops.pose_graph_optimize_batch(hip_ctx, ops.pose_graph_params(configs.get("kitti")["graph"]), g)
    rig.w.X[...] = g.X.cpu().numpy().reshape(rig.w.X.shape)
    assert g.result_of(1)["status"] == 0 and not np.array_equal(before[1], g.X[1].cpu().numpy())
    want = ref.unroll(rig.w, np.full((5, 24, 4, 4), -1.0, F))
    got = rig.sess.unroll(hip_ctx).cpu().numpy().reshape(5, 24, 4, 4)
    assert got.tobytes() == want.tobytes()


UNROLL_NODES = 5
# (B, frame_stride) and the n_frames of the runs: the unroll takes one thread per (sequence, frame) of a flat index over workgroups
# of 256 threads.  (1, 257): the second workgroup, of one row.  (3, 300): workgroups that hold the end of one sequence and the start
# of the next.  (2, 4541): the real length.  n_frames cover 0, 1, 256, 257 and frame_stride
UNROLL_SHAPES = [
    (1, 257, [(257,), (257,), (257,), (256,), (1,), (0,)]),
    (3, 300, [(300, 256, 257), (257, 300, 1), (0, 1, 300)]),
    (2, 4541, [(4541, 257), (256, 4541)]),
]


def _fill_log(rig, rng, run):
    """a hand-filled log on both sides: rigid logged poses, nodes 0 .. UNROLL_NODES - 1 with distinct node poses far from the
    identity and, in every workgroup of the unroll, a row whose node is -1 and a row whose node is node_stride.  A workgroup of a
    single row takes turns with `run`: a good node, -1, node_stride.  -> the flat rows with a node out of range"""
    import torch
    w = rig.w
    B, fs, ns = w.batch, w.frame_stride, w.node_stride
    for b in range(B):
        for n in range(ns):
            T = sc.rotation(rng.normal(size=3), rng.uniform(0.5, 3.0)) @ sc.rotation(rng.normal(size=3), rng.uniform(0.5, 3.0))
            T[:3, 3] = rng.normal(size=3) * 50.0
            w.X[b, n] = T
    pose = np.tile(np.eye(4, dtype=F), (B * fs, 1, 1))
    for i in range(B * fs):
        T = sc.rotation(rng.normal(size=3), rng.uniform(-3.0, 3.0))
        T[:3, 3] = rng.normal(size=3) * 5.0
        pose[i] = T.astype(F)
    w.frame_pose[...] = pose.reshape(B, fs, 4, 4)
    node = rng.integers(0, ns, B * fs).astype(np.int32)
    bad = []
    for lo in range(0, B * fs, 256):
        rows = min(256, B * fs - lo)
        if rows == 1:
            node[lo] = (ns - 1, -1, ns)[run % 3]  # the good node is not node 0, whose pose a wrong index would find
            if run % 3:
                bad.append(lo)
        else:
            at = rng.choice(rows, 2, replace=False) + lo
            node[at[0]], node[at[1]] = -1, ns
            bad += [int(at[0]), int(at[1])]
    w.frame_node[...] = node.reshape(B, fs)
    dev = rig.sess.frame_pose.device
    rig.sess.frame_pose.copy_(torch.from_numpy(w.frame_pose.reshape(B, fs, 16)).to(dev))
    rig.sess.frame_node.copy_(torch.from_numpy(w.frame_node).to(dev))
    rig.graphs.X.copy_(torch.from_numpy(w.X.reshape(B, ns, 16)).to(dev))
    return bad


@pytest.mark.parametrize("B,frame_stride,runs", UNROLL_SHAPES, ids=["1x257", "3x300", "2x4541"])
def test_unroll_over_more_than_one_workgroup(hip_ctx, B, frame_stride, runs):
    """bytes against the restatement; the sentinel wherever the rule writes nothing; and, independently of the restatement, every
    written entry within 8 * 2^-24 * sum |terms| of the float64 product of the node pose and the logged pose.  The terms of entry
    (i, k) are G_ij * P_jk over j < 3 and, in the translation column, G_i3: the kernel rounds G to float32 once, every product
    once and adds three times, five roundings a term, and 8 leaves room for their compounding"""
    import torch
    rig = Rig(B, frame_stride, 4, UNROLL_NODES, 2)
    rng = np.random.default_rng([B, frame_stride])
    sentinel = np.full((B, frame_stride, 4, 4), 0xA5A5A5A5, np.uint32)
    seen_workgroups = set()
    for run, n_frames in enumerate(runs):
        bad = _fill_log(rig, rng, run)
        assert len(set(rig.w.frame_node.reshape(-1).tolist()) & set(range(UNROLL_NODES))) == UNROLL_NODES
        rig.w.n_frames[...] = n_frames
        rig.sess.n_frames.copy_(torch.tensor(n_frames, dtype=torch.int32))
        rig.sess.trajectory.view(torch.uint8).fill_(0xA5)
        want = ref.unroll(rig.w, sentinel.view(F).copy())
        got = rig.sess.unroll(hip_ctx).cpu().numpy().reshape(B, frame_stride, 4, 4)
        assert got.tobytes() == want.tobytes(), (run, n_frames)
        # which rows are written, from the rule alone
        written = np.arange(frame_stride)[None, :] < np.asarray(n_frames)[:, None]
        written.reshape(-1)[bad] = False
        untouched = (got.view(np.uint32) == 0xA5A5A5A5).all(axis=(2, 3))
        assert np.array_equal(untouched, ~written), (run, n_frames)
        seen_workgroups.update((np.nonzero(written.reshape(-1))[0] // 256).tolist())
        # the float64 product
        G = rig.w.X[np.arange(B)[:, None], np.clip(rig.w.frame_node, 0, UNROLL_NODES - 1)]  # [B, fs, 4, 4] float64
        P = rig.w.frame_pose.astype(np.float64)
        product = G @ P
        terms = np.abs(G[..., :3, :3]) @ np.abs(P[..., :3, :])
        terms[..., 3] += np.abs(G[..., :3, 3])
        error = np.abs(got[..., :3, :].astype(np.float64) - product[..., :3, :])[written]
        bound = (8.0 * 2.0 ** -24) * terms[written]
        assert error.shape[0] == written.sum() and (error <= bound).all(), (run, n_frames, float((error / bound).max()))
        assert (got[written][:, 3] == np.array([0, 0, 0, 1], F)).all()
    assert seen_workgroups == set(range(-(-B * frame_stride // 256)))  # every workgroup of the launch has written rows


def test_batch_invariance(hip_ctx):
    """one sequence alone and the same sequence at slot 3 of B = 5 give the same bits"""
    frames = planted_inputs()
    alone = Rig(1, 24, 37, 3, 3, handover_stride=40)
    _planted_run(hip_ctx, alone, frames, pick=3)
    batch = Rig(5, 24, 37, 3, 3, handover_stride=40)
    _planted_run(hip_ctx, batch, frames)
    a, b = alone.device_arrays(), batch.device_arrays()
    for name in a:
        assert a[name][0].tobytes() == b[name][3].tobytes(), name


def test_threshold_edges(hip_ctx):
    angle, A, B = sc.cosine_edge(0.25)
    at, beyond = sc.translation([0, 0, -10.0]).astype(F), sc.translation([0, 0, -10.0]).astype(F)
    beyond[2, 3] = np.nextafter(F(-10), F(-11))
    one, none = np.ones(4, np.int32), np.zeros(4, np.int32)

    def frame_one(distance, ang, Xs):
        rig = Rig(len(Xs), 2, 4, 2, 2)
        n = len(Xs)
        eye = np.tile(np.eye(4, dtype=F), (n, 1, 1))
        rig.step(hip_ctx, distance, ang, eye, one[:n], none[:n], none[:n])
        rig.step(hip_ctx, distance, ang, np.array(Xs, F), one[:n], none[:n], none[:n])
        rig.assert_equal()
        return list(rig.sess.reason.cpu().numpy())

    # t2 == d2 and c == cos_a do not split, one ulp beyond each does (X = the pose's inverse: exact for these matrices)
    assert frame_one(10, float(angle), [at, beyond, A, B]) == [0, 1, 0, 1]
    # icl's 3 rad: a 2.9 rad turn stays, 5 m and an ulp goes; an angle >= pi never splits by rotation
    turn, half = sc.rotation([0, 1, 0], 2.9).astype(F), sc.rotation([0, 1, 0], np.pi).astype(F)
    far = sc.translation([0, 0, -5.0]).astype(F)
    far[2, 3] = np.nextafter(F(-5), F(-6))
    assert frame_one(5, 3, [turn, far, half]) == [0, 1, 1]
    assert frame_one(5, float(F(np.pi)), [turn, far, half]) == [0, 1, 0]
    assert frame_one(5, 4.0, [turn, far, half]) == [0, 1, 0]


@pytest.mark.parametrize("capacity", [300, 301, 303])
def test_map_reset_and_handover(hip_ctx, capacity):
    n_points = np.array([0, 1, 255, 256, 257, capacity, 100, 299], np.int32)
    rig = Rig(8, 2, capacity, 2, 2, handover_stride=capacity + 4)
    rng = np.random.default_rng(capacity)
    rig.set_map(coords=rng.normal(size=(8, capacity, 4)).astype(F), desc=rng.integers(0, 256, (8, capacity, 32), dtype=np.uint8),
                n_points=n_points, n_meas=rng.integers(1, 9, (8, capacity)).astype(np.uint32))
    rig.set_handover(0xCD, -3.25, 77, 123)
    eye = np.tile(np.eye(4, dtype=F), (8, 1, 1))
    X = eye.copy()
    X[:6] = sc.translation([0, 0, -11.0]).astype(F)  # sequences 0-5 split, 6 and 7 stay
    one, none = np.ones(8, np.int32), np.zeros(8, np.int32)
    rig.step(hip_ctx, 10, 0.25, eye, one, none, none)
    rig.set_map(n_points=n_points)
    rig.step(hip_ctx, 10, 0.25, X, one, none, none)
    rig.assert_equal()
    got = rig.device_arrays()
    assert list(got["reason"]) == [1] * 6 + [0, 0] and list(got["handover_n_query"]) == list(n_points[:6]) + [0, 0]
    for b in range(6):
        n = n_points[b]
        assert np.array_equal(got["handover_xyz"][b, :n], rig.w.coords[b, :n]) and (got["handover_xyz"][b, n:] == F(-3.25)).all()
        assert np.array_equal(got["handover_desc"][b, :n], rig.w.desc[b, :n]) and (got["handover_desc"][b, n:] == 0xCD).all()
        assert not got["n_meas"][b].any() and got["n_points"][b] == 0 and got["handover_graph_id"][b] == 0
    for b in (6, 7):
        assert (got["handover_xyz"][b] == F(-3.25)).all() and (got["handover_desc"][b] == 0xCD).all() and got["handover_graph_id"][b] == 123
        assert got["n_meas"][b].all() and got["n_points"][b] == n_points[b]


def test_errors(hip_ctx):
    far = sc.translation([0, 0, -11.0]).astype(F)[None]
    one, none = np.ones(1, np.int32), np.zeros(1, np.int32)
    # edge capacity: the second split finds no edge; frame capacity: the third frame finds no log row
    rig = Rig(1, 3, 4, 4, 1, handover_stride=4)
    for k in range(4):
        rig.step(hip_ctx, 10, 0.25, far, one, none, 5 * one)
        rig.assert_equal(k)
    assert rig.w.status[0] == ref.ERR_CAPACITY and rig.w.n_edges[0] == 1 and rig.w.n_frames[0] == 4
    # negative counters, one at a time, and a node outside the graph: nothing but the status moves
    for name, value in (("slot", -1), ("n_frames", -2), ("cur_node", -1), ("cur_node", 3), ("n_points", -1), ("n_points", 5), ("n_nodes", -1),
                        ("n_edges", -1)):
        rig = Rig(2, 3, 4, 4, 4, handover_stride=4)
        two = np.ones(2, np.int32)
        rig.step(hip_ctx, 10, 0.25, np.tile(far, (2, 1, 1)), two, 0 * two, two)
        holder = {"n_points": rig.maps, "n_nodes": rig.graphs, "n_edges": rig.graphs}.get(name, rig.sess)
        getattr(holder, name)[1] = value
        getattr(rig.w, name)[1] = value
        rig.set_handover(0x11, 1.0, 9, 9)
        rig.step(hip_ctx, 10, 0.25, np.tile(far, (2, 1, 1)), two, 0 * two, two)
        rig.assert_equal(name)
        assert list(rig.sess.status.cpu().numpy()) == [0, ref.ERR_RANGE] and rig.queries.n_query[1].item() == 0
    # call-level: a null mandatory pointer and a hand-over stride below the capacity; nothing is launched
    rig = Rig(1, 3, 8, 4, 4, handover_stride=8)
    rig.sess.status.fill_(55)
    p = ops.session_params(configs.get("kitti")["split"])
    lib = _lib.load()
    for field in ("pose", "X", "result", "n_meas", "graph_X", "Z", "handover_xyz"):
        d = rig.sess.descriptor()
        setattr(d, field, None)
        assert lib.prs_session_step_batch(hip_ctx._h, C.byref(p), C.byref(d)) == -1, field
    d = rig.sess.descriptor()
    d.handover_stride = 7
    assert lib.prs_session_step_batch(hip_ctx._h, C.byref(p), C.byref(d)) == ref.ERR_CAPACITY
    d = rig.sess.descriptor()
    d.omega = None
    assert lib.prs_session_step_batch(hip_ctx._h, C.byref(p), C.byref(d)) == -5  # information 0.1 needs omega
    d = rig.sess.descriptor()
    d.frame_pose = None
    assert lib.prs_session_unroll_batch(hip_ctx._h, C.byref(d), rig.sess.trajectory.data_ptr()) == -1
    hip_ctx.synchronize()
    assert rig.sess.status[0].item() == 55 and rig.sess.n_frames[0].item() == 0


def test_detector_handover(hip_ctx):
    """a finished map exported by a split gives the loop detector the same candidates, correspondences and verdict as the same map
    passed through upload()"""
    k = configs.get("kitti")
    rng = np.random.default_rng(77)
    n, cap = 220, 256
    xyz = np.stack([rng.uniform(-8, 8, n), rng.uniform(-2, 2, n), rng.uniform(3, 25, n)], axis=1).astype(F)
    desc = syn.random_descriptors(rng, n)
    db = ops.PlaceDatabase(hip_ctx)
    db.add(500, syn.random_descriptors(rng, 180), np.asarray(rng.normal(size=(180, 3)), F))
    db.add(501, desc, xyz)
    # the query: the planted map seen from a pose 0.3 m and 0.02 rad away, a few descriptor bits flipped
    T = sc.rotation([0, 1, 0.2], 0.02)
    T[:3, 3] = [0.3, 0.0, -0.1]
    q_xyz = (xyz.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    q_desc = desc.copy()
    q_desc[np.arange(n), rng.integers(0, 32, n)] ^= np.uint8(1) << rng.integers(0, 8, n).astype(np.uint8)
    P = ops.place_params(k["place"], max_candidates=2, minimum_age_difference_to_candidates=0)
    bf, pa = ops.bruteforce_params(k["loop"]["maximum_descriptor_distance"], 0.9), ops.point_align_params(k["loop"])
    direct = ops.LoopDetectorBatch(0, db, 1, cap, 2)
    direct.upload(0, 7, q_desc, q_xyz)
    direct.run(hip_ctx, P, bf, pa)
    want = direct.result_of(0)
    assert want["candidates"] == [1] and len(want["accepted"]) == 1
    # the same map as local map 0 of a session; frame 1 moves 11 m: the split exports it as the query of graph id 7 + node 0
    import torch
    via = ops.LoopDetectorBatch(0, db, 1, cap, 2)
    maps, frames = ops.MapBatch(0, 1, cap, 1, 4, 1, 1), ops.AlignFrames(0, 1, 1, 1)
    graphs = ops.PoseGraphBatch(0, 1, 4, 4, envelope_blocks=16)
    base = torch.full((1,), 7, dtype=torch.int64, device=maps.coords.device)
    sess = ops.SessionBatch(0, maps, frames, graphs, 4, handover=via.queries, graph_id_base=base)
    sp = ops.session_params(k["split"])
    sess.step(hip_ctx, sp)
    maps.coords[0, :n, :3] = torch.from_numpy(q_xyz).to(maps.coords.device)
    maps.desc[0, :n] = torch.from_numpy(q_desc).to(maps.desc.device)
    maps.n_points[0] = n
    frames.X[0] = torch.from_numpy(sc.translation([0, 0, -11.0]).astype(F).reshape(16)).to(frames.X.device)
    frames.result.view(torch.int32)[0, ops.AlignResult.status.offset // 4] = 1
    sess.step(hip_ctx, sp)
    assert sess.result_of(0)["reason"] == ops.SESSION_SPLIT_VIEWPOINT and via.queries.graph_id[0].item() == 7
    via.run(hip_ctx, P, bf, pa)
    got = via.result_of(0)
    assert got["candidates"] == want["candidates"] and got["accepted"] == want["accepted"]
    assert got["search"]["status"] == want["search"]["status"] and np.array_equal(got["search"]["counts"], want["search"]["counts"])
    for a, b in zip(got["search"]["corr"], want["search"]["corr"]):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(got["poses"], want["poses"]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    # the next frame does not split: the query slot is emptied and the search answers it with "empty input"
    frames.X.copy_(sess.prediction)  # pose = prediction * X^-1: back at the new map's origin
    sess.step(hip_ctx, sp)
    assert sess.result_of(0)["reason"] == ops.SESSION_NO_SPLIT
    via.run(hip_ctx, P, bf, pa)
    empty = via.result_of(0)
    assert empty["candidates"] == [] and empty["search"]["status"] == 1
    db.close()
