"""Map re-entry on the device (ops.MapArchive, ops.ReentryBatch: prs_session_step_archive_batch, prs_session_reenter_batch) against
its numpy restatement (tests/reentry_ref.py on top of tests/session_ref.py).  Every compared array is byte-equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import reentry_ref as rr
import session_cases as sc
import session_ref as sr
from srrg2_proslam_amd import _lib, configs, ops, synthetic as syn
from test_session_gpu import planted_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
F = np.float32
KITTI = rr.params(10, 25, 0.5, 5)  # configs.REENTRY["kitti"]
FAR = sc.translation([0, 0, -11.0]).astype(F)


def _push(t, a):
    import torch
    a = np.ascontiguousarray(a)
    t.copy_(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(t.device).reshape(t.shape))


class Rig:
    """a ReentryBatch over small maps, aligner outputs, graphs, a bank detector whose outputs the tests plant, and the restatement's
    arrays that mirror all of it"""

    def __init__(self, ctx, B, frame_stride, capacity, node_stride, edge_stride, handover_stride, slot_stride=3, max_measurements=0,
                 max_frames=4, max_candidates=3, map_stride=4, measurement_stride=1, with_omega=True):
        self.ctx, self.B = ctx, B
        self.maps = ops.MapBatch(0, B, capacity, max_measurements, max_frames, measurement_stride, measurement_stride)
        self.frames = ops.AlignFrames(0, B, 1, 1)
        self.graphs = ops.PoseGraphBatch(0, B, node_stride, edge_stride, envelope_blocks=4 * node_stride, with_omega=with_omega)
        self.bank = ops.PlaceBank(ctx, B, map_stride, 2 * handover_stride)
        self.det = ops.BankDetectorBatch(0, self.bank, B, handover_stride, max_candidates)
        self.queries = self.det.queries
        self.sess = ops.SessionBatch(0, self.maps, self.frames, self.graphs, frame_stride, handover=self.queries)
        self.arch = ops.MapArchive(0, self.maps, node_stride, slot_stride, with_history=max_measurements > 0)
        self.rb = ops.ReentryBatch(self.sess, self.maps, self.det, self.arch)
        self.w = sr.World(B, frame_stride, capacity, node_stride, edge_stride, handover_stride, with_omega)
        self.live = rr.LiveMaps(B, capacity, max_measurements, max_frames)
        self.a = rr.Archive(B, capacity, slot_stride, node_stride, max_measurements, max_frames if max_measurements > 0 else 0)
        self.d = rr.Detector(B, max_candidates, map_stride, self.rb.corr_stride)
        self.out = rr.Reentry(B, self.rb.corr_stride)
        for name, arr in self.out.arrays().items():
            arr[...] = getattr(self.rb, name).cpu().numpy().reshape(arr.shape)
        self.information = {} if with_omega else dict(split_information=1.0, lost_information=1.0)

    def close(self):
        self.bank.close()

    # ---- the same contents on both sides
    def set_map(self, **arrays):
        for name, value in arrays.items():
            holder = self.w if name in ("coords", "desc", "n_points", "n_meas") else self.live
            getattr(holder, name)[...] = value
            _push(getattr(self.maps, name), getattr(holder, name))

    def set_stats(self, rng, sel=lambda a: a, rows=5):
        """random statistics arrays (and history), what a merger would have left; sel picks the sequences of a smaller rig"""
        cap, lv = self.w.capacity, self.live
        mm, mf = lv.meas.shape[2], lv.poses.shape[1]
        self.set_map(state=sel(rng.normal(size=(rows, cap, 4)).astype(F)), covariance=sel(rng.normal(size=(rows, cap, 9)).astype(F)),
                     n_opt=sel(rng.integers(0, 50, (rows, cap)).astype(np.uint32)), inlier=sel(rng.integers(0, 2, (rows, cap)).astype(np.uint8)),
                     meas=sel(rng.integers(-2 ** 30, 2 ** 30, (rows, cap, mm, rr.MEAS_WORDS)).astype(np.int32)),
                     poses=sel(rng.normal(size=(rows, mf, rr.POSE_WORDS)).astype(F)))

    def set_handover(self, desc_byte, xyz_value, n_query, graph_id):
        w, q = self.w, self.queries
        w.handover_desc[...], w.handover_xyz[...], w.handover_n_query[...], w.handover_graph_id[...] = desc_byte, xyz_value, n_query, graph_id
        q.desc.fill_(desc_byte)
        q.xyz.fill_(xyz_value)
        q.n_query.fill_(n_query)
        q.graph_id.fill_(graph_id)

    def set_alignment(self, X, status, warnings, n_corr):
        f = self.frames
        _push(f.X, np.ascontiguousarray(X, F).reshape(self.B, 16))
        raw = np.zeros((self.B, C.sizeof(ops.AlignResult)), np.uint8)
        words = raw.view(np.int32)
        words[:, ops.AlignResult.status.offset // 4] = status
        words[:, ops.AlignResult.warnings.offset // 4] = warnings
        _push(f.result, raw)
        _push(f.n_corr, np.asarray(n_corr, np.int32))

    def step(self, distance, angle, X, status, warnings, n_corr):
        self.set_alignment(X, status, warnings, n_corr)
        self.rb.step(self.ctx, ops.session_params(dict(local_map_distance=distance, local_map_angle_distance_radians=angle), **self.information))
        rr.step_archive(self.w, self.live, self.a, distance, angle, X, status, warnings, n_corr, **self.information)

    def far_step(self, status=None, X=None):
        one, none = np.ones(self.B, np.int32), np.zeros(self.B, np.int32)
        X = np.tile(FAR, (self.B, 1, 1)) if X is None else X
        self.step(10, 0.25, X, one if status is None else status, none, one)

    def push_detector(self):
        d, det, pairs = self.d, self.det, self.det.closures.pairs
        _push(det.links.candidates_flat, d.candidates_flat)
        _push(self.bank.node_of_map, d.node_of_map)
        _push(pairs.result, d.result)
        _push(pairs.X, d.X.reshape(-1, 16))
        _push(pairs.corr, d.corr)
        _push(pairs.n_corr, d.n_corr)

    def reenter(self, P=KITTI):
        self.push_detector()
        self.rb.reenter(self.ctx, ops.reentry_params(P))
        rr.reenter(self.w, self.live, self.a, self.d, self.out, P)

    # ---- what is compared
    def device_arrays(self):
        s, m, g, q = self.sess, self.maps, self.graphs, self.queries
        out = dict(pose=s.pose, prev=s.prev, prediction=s.prediction, slot=s.slot, cur_node=s.cur_node, n_frames=s.n_frames,
                   frame_node=s.frame_node, frame_pose=s.frame_pose, status=s.status, reason=s.reason, n_corr_merge=s.n_corr_merge,
                   n_points=m.n_points, n_meas=m.n_meas, frame=m.frame, measurement_in_world=m.measurement_in_world,
                   measurement_in_scene=m.measurement_in_scene, X=g.X, fixed=g.fixed, n_nodes=g.n_nodes, n_edges=g.n_edges, src=g.src,
                   dst=g.dst, Z=g.Z, handover_desc=q.desc, handover_xyz=q.xyz, handover_n_query=q.n_query, handover_graph_id=q.graph_id,
                   coords=m.coords, desc=m.desc)
        if g.omega is not None:
            out["omega"] = g.omega
        return {k: v.cpu().numpy() for k, v in out.items()}

    def live_arrays(self):
        m = self.maps
        return {k: getattr(m, k).cpu().numpy() for k in ("state", "covariance", "n_opt", "inlier", "meas", "poses", "n_measured")}

    def archive_arrays(self):
        return {k: getattr(self.arch, k).cpu().numpy() for k in self.a.arrays()}

    def reentry_arrays(self):
        return {k: getattr(self.rb, k).cpu().numpy() for k in self.out.arrays()}

    def all_arrays(self):
        out = self.device_arrays()
        out.update({"live." + k: v for k, v in self.live_arrays().items()})
        out.update({"archive." + k: v for k, v in self.archive_arrays().items()})
        out.update({"reentry." + k: v for k, v in self.reentry_arrays().items()})
        return out

    def assert_equal(self, what=""):
        for name, got in self.device_arrays().items():
            assert got.tobytes() == np.ascontiguousarray(getattr(self.w, name)).tobytes(), (what, name)
        for name, got in self.live_arrays().items():
            assert got.tobytes() == np.ascontiguousarray(getattr(self.live, name)).tobytes(), (what, "live", name)
        for name, got in self.archive_arrays().items():
            assert got.tobytes() == np.ascontiguousarray(getattr(self.a, name)).tobytes(), (what, "archive", name)
        for name, got in self.reentry_arrays().items():
            assert got.tobytes() == np.ascontiguousarray(getattr(self.out, name)).tobytes(), (what, "reentry", name)


# ---- 1. the archive step equals the plain step, plus the archive
def test_planted_sequences_through_the_archive_step(hip_ctx):
    frames = planted_inputs()
    rig = Rig(hip_ctx, 5, 24, 37, 3, 3, handover_stride=40, slot_stride=3, max_measurements=2, max_frames=4)
    rng = np.random.default_rng(5)
    rig.set_map(coords=rng.normal(size=(5, 37, 4)).astype(F), desc=rng.integers(0, 256, (5, 37, 32), dtype=np.uint8))
    rig.set_handover(0xAB, 7.5, -3, -9)
    splits = 0
    for k, (X, status, warnings, n_corr) in enumerate(frames):
        rig.set_map(n_points=np.full(5, 10 + k, np.int32), n_meas=rng.integers(1, 5, (5, 37)).astype(np.uint32))
        rig.set_stats(rng)
        before = rig.archive_arrays()
        rig.step(10, 0.25, X, status, warnings, n_corr)
        rig.assert_equal("frame %d" % k)
        after = rig.archive_arrays()
        for b in np.nonzero(rig.w.reason == sr.NO_SPLIT)[0]:  # a frame without a split leaves the sequence's archive bytes alone
            for name in after:
                if name != "status":
                    assert after[name][b].tobytes() == before[name][b].tobytes(), (k, b, name)
        splits += int((rig.w.reason != sr.NO_SPLIT).sum())
    assert splits == 8 and rig.a.n_slots.tolist() == [2, 2, 0, 2, 2] and not rig.a.status.any()
    assert rig.a.slot_of_node.tolist() == [[0, 1, -1], [0, 1, -1], [-1, -1, -1], [0, 1, -1], [0, 1, -1]]
    assert rig.a.n_points[0].tolist() == [10 + 12, 10 + 23, 0] and rig.a.next_frame[0].tolist() == [12, 11, 0]
    rig.close()


@pytest.mark.parametrize("max_measurements", [0, 2])
@pytest.mark.parametrize("capacity", [300, 301, 303])
def test_archive_copy_and_reset_at_the_alignment_edges(hip_ctx, capacity, max_measurements):
    n_points = np.array([0, 1, 255, 256, 257, capacity, 100, 299], np.int32)
    rig = Rig(hip_ctx, 8, 2, capacity, 2, 2, handover_stride=capacity + 4, slot_stride=2, max_measurements=max_measurements, max_frames=3)
    rng = np.random.default_rng(capacity)
    rig.set_map(coords=rng.normal(size=(8, capacity, 4)).astype(F), desc=rng.integers(0, 256, (8, capacity, 32), dtype=np.uint8),
                n_points=n_points, n_meas=rng.integers(1, 9, (8, capacity)).astype(np.uint32))
    rig.set_stats(rng, rows=8)
    rig.set_handover(0xCD, -3.25, 77, 123)
    eye = np.tile(np.eye(4, dtype=F), (8, 1, 1))
    X = eye.copy()
    X[:6] = FAR  # sequences 0-5 split, 6 and 7 stay
    one, none = np.ones(8, np.int32), np.zeros(8, np.int32)
    rig.step(10, 0.25, eye, one, none, none)
    rig.set_map(n_points=n_points)
    rig.step(10, 0.25, X, one, none, none)
    rig.assert_equal()
    got = rig.archive_arrays()
    assert got["n_slots"].tolist() == [1] * 6 + [0, 0] and got["n_points"][:, 0].tolist() == n_points[:6].tolist() + [0, 0]
    for b in range(6):
        n = n_points[b]
        assert got["n_meas"][b, 0, :n].all() and not got["n_meas"][b, 0, n:].any() and not rig.maps.n_meas[b].any().item()
        assert np.array_equal(got["covariance"][b, 0, :n], rig.live.covariance[b, :n]) and not got["covariance"][b, 0, n:].any()
    rig.close()


# ---- 2. overwrite and full
def _plant_good(rig, b, k=0, map_index=0, node=0, ni=40, nc=50, chi=40.0, X=None, accepted=1, corr=None):
    X = sc.translation([0, 0, 19.0]) if X is None else X
    rig.d.plant(b, k, map_index, node, X, ni, nc, chi, accepted, corr)


def _walk(rig, rng, lost=(), stay=(), rows=None, sel=lambda a: a):
    """frame 0, a split into node 1 (map 0 archived), a split into node 2 (map 1 archived): m = 2, f = 1.  Sequences in `lost` lose
    track at the second split, those in `stay` do not split there."""
    B, cap = rig.B, rig.w.capacity
    rows = B if rows is None else rows
    rig.set_map(coords=sel(rng.normal(size=(rows, cap, 4)).astype(F)), desc=sel(rng.integers(0, 256, (rows, cap, 32), dtype=np.uint8)))
    rig.set_stats(rng, sel, rows)
    rig.far_step()
    rig.set_map(n_points=sel(np.arange(rows, dtype=np.int32) % 7 + 20), n_meas=sel(rng.integers(1, 5, (rows, cap)).astype(np.uint32)))
    rig.far_step()
    rig.set_map(coords=sel(rng.normal(size=(rows, cap, 4)).astype(F)), n_points=sel(np.arange(rows, dtype=np.int32) % 5 + 9),
                n_meas=sel(rng.integers(1, 5, (rows, cap)).astype(np.uint32)))
    rig.set_stats(rng, sel, rows)
    status = np.ones(B, np.int32)
    X = np.tile(FAR, (B, 1, 1))
    for b in lost:
        status[b] = 0
    for b in stay:
        X[b] = rig.w.prediction[b]  # pose = prediction * X^-1: back at the map's origin
    rig.far_step(status, X)
    # what the frame's merge would leave behind in the map that follows: measurement counts that a re-entry has to clear
    rig.set_map(n_meas=sel(rng.integers(1, 5, (rows, cap)).astype(np.uint32)))
    rig.assert_equal("walk")


def test_a_reentered_map_overwrites_its_slot_and_a_full_archive_refuses(hip_ctx):
    rng = np.random.default_rng(21)
    rig = Rig(hip_ctx, 2, 6, 40, 4, 6, handover_stride=40, slot_stride=3, max_measurements=2)
    _walk(rig, rng)
    _plant_good(rig, 0)
    rig.reenter()
    rig.assert_equal("re-entry")
    assert rig.out.reentered.tolist() == [1, 0] and rig.w.cur_node.tolist() == [0, 2] and rig.a.n_slots.tolist() == [2, 2]
    rig.set_map(n_points=np.array([31, 12], np.int32))  # the closure merger added landmarks to map 0; sequence 1 grew map 2
    rig.set_stats(rng, rows=2)
    rig.far_step()
    rig.assert_equal("finished again")
    assert rig.a.n_slots.tolist() == [2, 3] and rig.a.slot_of_node[0].tolist() == [0, 1, -1, -1] and rig.a.n_points[0, 0] == 31
    assert rig.a.slot_of_node[1].tolist() == [0, 1, 2, -1] and not rig.a.status.any()
    rig.close()
    # slot_stride 1: the second distinct map finds the archive full, the split itself is the reference's
    rig = Rig(hip_ctx, 2, 6, 40, 4, 6, handover_stride=40, slot_stride=1)
    rig.set_map(coords=rng.normal(size=(2, 40, 4)).astype(F), n_points=np.array([7, 8], np.int32))
    rig.far_step()
    rig.far_step()
    assert rig.a.status.tolist() == [0, 0] and rig.a.n_slots.tolist() == [1, 1]
    rig.set_map(n_points=np.array([9, 10], np.int32))
    before = rig.archive_arrays()
    rig.far_step()
    rig.assert_equal("full")
    after = rig.archive_arrays()
    assert rig.a.status.tolist() == [sr.ERR_CAPACITY] * 2 and rig.w.reason.tolist() == [1, 1] and rig.w.n_nodes.tolist() == [3, 3]
    assert all(after[k].tobytes() == before[k].tobytes() for k in after if k != "status")
    rig.close()


# ---- 3. selection
def _selection_cases():
    """(name, plants(rig, b), expected reentered, expected merge_transform z or None, lost, stay, drop map 0's slot)"""
    G = lambda z: sc.translation([0, 0, z])  # noqa: E731  Z_e = (0, 0, 22): P = (0, 0, 22 - z)
    at, beyond = G(12.0), G(12.0)
    beyond[2, 3] = np.nextafter(F(12), F(0))
    cases = [
        ("nothing accepted", lambda r, b: [_plant_good(r, b, k, k, 0, accepted=0) for k in range(3)], 0, None),
        ("inliers at the minimum", lambda r, b: _plant_good(r, b, ni=25, nc=40, chi=25.0), 1, 19.0),
        ("inliers one below", lambda r, b: _plant_good(r, b, ni=24, nc=40, chi=24.0), 0, None),
        ("ratio at the minimum", lambda r, b: _plant_good(r, b, ni=32, nc=64, chi=32.0), 1, 19.0),
        ("ratio below", lambda r, b: _plant_good(r, b, ni=32, nc=65, chi=32.0), 0, None),
        ("chi at the maximum", lambda r, b: _plant_good(r, b, ni=32, nc=40, chi=160.0), 1, 19.0),
        ("chi one float above", lambda r, b: _plant_good(r, b, ni=32, nc=40, chi=np.nextafter(F(160), F(200))), 0, None),
        ("t2 at the squared limit", lambda r, b: _plant_good(r, b, X=at), 1, 12.0),
        ("t2 one float beyond", lambda r, b: _plant_good(r, b, X=beyond), 0, None),
        ("more inliers win", lambda r, b: [_plant_good(r, b, 0, 0, 0, ni=30, X=G(18.0)), _plant_good(r, b, 1, 1, 0, ni=40, nc=60, X=G(17.0))], 1, 17.0),
        ("a tie goes to the lower slot", lambda r, b: [_plant_good(r, b, 0, 0, 0, ni=30, X=G(18.0)), _plant_good(r, b, 2, 1, 0, ni=30, X=G(17.0))], 1, 18.0),
        ("lost", lambda r, b: _plant_good(r, b), 0, None),
        ("no split", lambda r, b: _plant_good(r, b), 0, None),
        ("the node has no slot", lambda r, b: _plant_good(r, b), 0, None),
        ("no candidate", lambda r, b: _plant_good(r, b, map_index=-1), 0, None),
        ("the candidate is the finished map", lambda r, b: _plant_good(r, b, node=1), 0, None),
    ]
    return cases


def _selection_run(ctx, P, pick=None):
    cases = _selection_cases()
    names = [c[0] for c in cases]
    n = len(cases)
    sel = (lambda a: a) if pick is None else (lambda a: a[pick: pick + 1])
    idx = list(range(n)) if pick is None else [pick]
    rig = Rig(ctx, len(idx), 4, 40, 4, 6, handover_stride=40, slot_stride=2, max_measurements=2)
    _walk(rig, np.random.default_rng(33), lost=[i for i, j in enumerate(idx) if names[j] == "lost"],
          stay=[i for i, j in enumerate(idx) if names[j] == "no split"], rows=n, sel=sel)
    corr_rng = np.random.default_rng(34)
    corrs = corr_rng.integers(0, 9, (n, 3, 5, 3)).astype(np.int32)
    for i, j in enumerate(idx):
        cases[j][1](rig, i)
        for k in range(3):  # every slot carries a matcher vector; the winner's is the one that travels
            rig.d.corr[i * 3 + k, :5], rig.d.n_corr[i * 3 + k] = corrs[j, k], 3 + k
        if names[j] == "the node has no slot":
            rig.a.slot_of_node[i, 0] = -1
            rig.arch.slot_of_node[i, 0] = -1
    before = rig.all_arrays()
    rig.reenter(P)
    return rig, before, cases, idx


def test_selection(hip_ctx):
    rig, before, cases, idx = _selection_run(hip_ctx, KITTI)
    rig.assert_equal("selection")
    after = rig.all_arrays()
    for b, (name, _, _, _) in enumerate(cases):  # the odometry edge the cases' transforms are planted against
        if name not in ("lost", "no split"):
            assert rig.w.Z[b, 1, :3, 3].tolist() == [0, 0, 22] and rig.w.src[b, 1] == 1 and rig.w.dst[b, 1] == 2, name
    for b, (name, _, want, z) in enumerate(cases):
        assert int(rig.out.reentered[b]) == want and int(rig.out.status[b]) == sr.OK, name
        if want:
            assert rig.out.merge_transform[b, 2, 3] == F(z) and rig.w.cur_node[b] == 0 and rig.out.gate[b, rr.R_ACCEPTED] == 1, name
            k = {19.0: 0, 12.0: 0, 17.0: 1, 18.0: 0}[z]
            assert rig.out.merge_n_corr[b] == 3 + k and np.array_equal(rig.out.merge_corr[b, : 3 + k], rig.d.corr[b * 3 + k, : 3 + k]), name
        else:  # the session, the map, the graph and the archive: not a byte moves
            for key in after:
                if not key.startswith("reentry."):
                    assert after[key][b].tobytes() == before[key][b].tobytes(), (name, key)
            assert rig.out.gate[b, rr.R_ACCEPTED] == 0, name
    # the planted edges are what they claim: t2 == 100 exactly, and the next float beyond
    assert rr.translation2(sc.translation([0, 0, 10.0])) == F(100) and rr.translation2(sc.translation([0, 0, float(np.nextafter(F(10), F(11)))])) > F(100)
    batch = rig.all_arrays()
    rig.close()
    # every case alone gives the bytes it gives in the batch
    for j in range(len(cases)):
        alone, _, _, _ = _selection_run(hip_ctx, KITTI, pick=j)
        alone.assert_equal(cases[j][0])
        got = alone.all_arrays()
        for key in got:
            assert got[key][0].tobytes() == batch[key][j].tobytes(), (cases[j][0], key)
        alone.close()


def test_selection_one_float_beyond_each_float_threshold(hip_ctx):
    names = [c[0] for c in _selection_cases()]
    i_ratio, i_chi = names.index("ratio at the minimum"), names.index("chi at the maximum")
    up = lambda v: float(np.nextafter(F(v), F(np.inf)))  # noqa: E731
    down = lambda v: float(np.nextafter(F(v), F(-np.inf)))  # noqa: E731
    for P, flips in ((rr.params(10, 25, up(0.5), 5), [i_ratio]), (rr.params(10, 25, 0.5, down(5)), [i_chi])):
        rig, _, cases, _ = _selection_run(hip_ctx, P)
        rig.assert_equal()
        want = [0 if b in flips else c[2] for b, c in enumerate(cases)]
        assert rig.out.reentered.tolist() == want
        rig.close()
    # a squared limit one float below 100 turns the sequence at exactly 10 m away
    P = rr.params(down(10), 25, 0.5, 5)
    rig, _, cases, _ = _selection_run(hip_ctx, P)
    rig.assert_equal()
    assert rig.out.reentered.tolist() == [0 if c[0] == "t2 at the squared limit" else c[2] for c in cases]
    rig.close()


# ---- 4. graph fix-up
@pytest.mark.parametrize("with_omega", [True, False])
@pytest.mark.parametrize("n_closures", [0, 1, 2])
def test_graph_fix_up(hip_ctx, n_closures, with_omega):
    rng = np.random.default_rng(40 + n_closures)
    rig = Rig(hip_ctx, 2, 4, 24, 4, 6, handover_stride=24, slot_stride=2, with_omega=with_omega)
    _walk(rig, rng)
    w, g = rig.w, rig.graphs
    for j in range(n_closures):  # what prs_pose_graph_append_closures leaves behind the odometry edge: from f to the candidate's node
        e = 2 + j
        w.src[:, e], w.dst[:, e], w.Z[:, e] = 1, 0, rng.normal(size=(2, 4, 4)).astype(F)
        if with_omega:
            w.omega[:, e] = rng.normal(size=(2, 6, 6)).astype(F)
    w.n_edges[:] = 2 + n_closures
    for name, t in (("src", g.src), ("dst", g.dst), ("Z", g.Z), ("n_edges", g.n_edges)) + ((("omega", g.omega),) if with_omega else ()):
        _push(t, getattr(w, name))
    before = {k: v.copy() for k, v in rig.device_arrays().items()}
    _plant_good(rig, 0)
    rig.reenter()
    rig.assert_equal()
    got = rig.device_arrays()
    assert got["n_nodes"].tolist() == [2, 3] and got["n_edges"].tolist() == [1 + n_closures, 2 + n_closures]
    keep = [0] + list(range(2, 2 + n_closures))
    for name in ("src", "dst", "Z") + (("omega",) if with_omega else ()):
        assert got[name][0, : len(keep)].tobytes() == before[name][0, keep].tobytes(), name
        assert got[name][1].tobytes() == before[name][1].tobytes(), name
    assert got["frame_node"].tobytes() == before["frame_node"].tobytes()  # the split frame stays logged against f
    rig.close()


# ---- 5. restore
def _measurements(rig, rng, n):
    """n stereo measurements per sequence (uL, vL, uR, vR) on the kitti canvas, the same on both sides"""
    B = rig.B
    uv = np.zeros((B, rig.maps.measurement_stride, 4), F)
    uv[:, :n, 0], uv[:, :n, 1] = rng.uniform(100, 1100, (B, n)), rng.uniform(30, 340, (B, n))
    uv[:, :n, 2], uv[:, :n, 3] = uv[:, :n, 0] - rng.uniform(8, 40, (B, n)).astype(F), uv[:, :n, 1]
    _push(rig.maps.measurement, uv)
    _push(rig.maps.measurement_desc, rng.integers(0, 256, (B, rig.maps.measurement_stride, 32), dtype=np.uint8))
    rig.set_map(n_measured=np.full(B, n, np.int32))


@pytest.mark.parametrize("max_measurements", [0, 2])
def test_restore_and_the_disarmed_regular_merge(hip_ctx, max_measurements):
    from bench_merge import merger_params
    mp = merger_params(configs.get("kitti"), ops.EST_WEIGHTED_MEAN)
    runs = []
    for reentering in (True, False):
        rng = np.random.default_rng(50)
        rig = Rig(hip_ctx, 3, 4, 301, 4, 6, handover_stride=304, slot_stride=2, max_measurements=max_measurements, max_frames=6,
                  measurement_stride=8)
        _walk(rig, rng)
        _measurements(rig, rng, 6)
        if reentering:
            _plant_good(rig, 0)
            _plant_good(rig, 2, accepted=0)
        rig.reenter()
        rig.assert_equal()
        if reentering:
            n = int(rig.a.n_points[0, 0])
            assert rig.out.reentered.tolist() == [1, 0, 0] and n == 20 and rig.w.n_points.tolist() == [20, 0, 0]
            frame = int(rig.a.next_frame[0, 0]) if max_measurements else 0
            assert (int(rig.w.frame[0]), int(rig.w.slot[0])) == (frame, frame + 1) and frame == (1 if max_measurements else 0)
            got = rig.maps.n_meas[0].cpu().numpy()
            assert not got[n:].any() and bool(got[:n].all()) == bool(max_measurements)
            assert rig.live.n_measured.tolist() == [0, 6, 6]
        before = rig.all_arrays()
        ops.merge_batch(hip_ctx, mp, rig.maps)
        after = rig.all_arrays()
        assert (rig.maps.result[:, 2].cpu().numpy() >= 0).all()
        if reentering:  # the regular merge adds nothing to the re-entered map
            for key in ("n_points", "coords", "desc", "n_meas", "live.state", "live.covariance", "live.n_opt", "live.inlier", "live.meas"):
                assert after[key][0].tobytes() == before[key][0].tobytes(), key
            assert rig.maps.result[0].cpu().numpy().tolist()[:2] == [0, 0]
        assert (after["n_points"][1:] > before["n_points"][1:]).all()  # the neighbours' frames seed their new maps
        runs.append(after)
        rig.close()
    for key in runs[0]:  # the neighbours behave as in a batch in which nobody re-enters
        if not key.startswith("reentry."):
            assert runs[0][key][1:].tobytes() == runs[1][key][1:].tobytes(), key


# ---- 6. the chain, end to end
class Chain:
    """B = 3 sequences through archive step, bank detector, append_closures, optimiser, re-entry, closure merger and merger.  Sequence 0
    sees 60 landmarks from its first map's origin, walks 11.5 m ahead (a split; the new map holds the same landmarks and 12 more),
    and walks back to 0.3 m from where it started: the split there finds the first map and re-enters it.  Sequence 1 walks on through
    places that share nothing, sequence 2 stands still.  The maps' contents are planted where a merger would have left them."""

    N, EXTRA, CAP, FRAMES = 60, 12, 128, 5

    def __init__(self, ctx, reentry=True):
        import torch
        self.ctx, self.reentry = ctx, reentry
        k = configs.get("kitti")
        B, cap = 3, self.CAP
        self.maps = ops.MapBatch(0, B, cap, 0, 8, 1, 1)
        self.frames = ops.AlignFrames(0, B, 1, 1)
        self.graphs = ops.PoseGraphBatch(0, B, 8, 12, envelope_blocks=36)
        self.bank = ops.PlaceBank(ctx, B, 4, 4 * cap)
        self.det = ops.BankDetectorBatch(0, self.bank, B, cap, 2)
        self.sess = ops.SessionBatch(0, self.maps, self.frames, self.graphs, self.FRAMES, handover=self.det.queries)
        self.arch = ops.MapArchive(0, self.maps, 8, 4)
        self.rb = ops.ReentryBatch(self.sess, self.maps, self.det, self.arch)
        self.P = ops.place_params(k["place"], max_candidates=2, minimum_age_difference_to_candidates=0)
        self.bf, self.pa = ops.bruteforce_params(k["loop"]["maximum_descriptor_distance"], 0.9), ops.point_align_params(k["loop"], robustifier=_lib.ROBUSTIFIER_SATURATED)
        self.gp, self.sp = ops.pose_graph_params(k["graph"]), ops.session_params(k["split"])
        self.rp = ops.reentry_params(configs.REENTRY["kitti"])
        self.cp = ops.closure_merger_params(k["closure_merger"], k["camera"])
        self.mp = __import__("bench_merge").merger_params(k, ops.EST_WEIGHTED_MEAN)
        rng = np.random.default_rng(61)
        n, m = self.N, self.N + self.EXTRA
        place = lambda cnt: np.stack([rng.uniform(-8, 8, cnt), rng.uniform(-2, 2, cnt), rng.uniform(16, 40, cnt)], axis=1).astype(F)  # noqa: E731
        xyz, desc = place(m), syn.random_descriptors(rng, m)
        seen_again = desc.copy()
        seen_again[np.arange(m), rng.integers(0, 32, m)] ^= np.uint8(1) << rng.integers(0, 8, m).astype(np.uint8)
        ahead = xyz.copy()
        ahead[:, 2] -= F(11.5)
        # per sequence, per frame: the alignment X (pose = prediction * X^-1) and the map contents planted after the frame
        T = lambda z: sc.translation([0, 0, z]).astype(F)  # noqa: E731
        other = [(place(40), syn.random_descriptors(rng, 40)) for _ in range(3)]
        self.X = [[T(0), T(-11.5), T(22.7), None, None], [T(0), T(-11.5), T(-11.5), T(-11.5), None], [T(0)] * 5]
        self.plant = [[(xyz[:n], desc[:n]), (ahead, seen_again), None, None, None], [other[0], other[1], other[2], None, None], [other[0]] + [None] * 4]
        self.log = []
        self.dev = self.maps.coords.device
        self.torch = torch

    def close(self):
        self.bank.close()

    def upload(self, k):
        """the frame's alignments; X = None: the session's own prediction, copied on the device -- pose = prediction * X^-1 is then
        the map's origin, whatever the prediction was"""
        torch = self.torch
        for b in range(3):
            X = self.X[b][k]
            if X is None:
                self.frames.X[b].copy_(self.sess.prediction[b])
            else:
                self.frames.X[b].copy_(torch.from_numpy(X.reshape(16)).to(self.dev))
            self.frames.result.view(torch.int32)[b, ops.AlignResult.status.offset // 4] = 1

    def launch(self):
        """the per-frame chain: plain launches on the context's stream"""
        ctx = self.ctx
        if self.reentry:
            self.rb.step(ctx, self.sp)
        else:
            self.sess.step(ctx, self.sp)
        self.det.run(ctx, self.P, self.bf, self.pa)
        self.graphs.append_closures(ctx, self.det.view, *self.det.node_maps())
        ops.pose_graph_optimize_batch(ctx, self.gp, self.graphs)
        if self.reentry:
            self.rb.reenter(ctx, self.rp)
            ops.closure_merge_batch(ctx, self.cp, self.rb.merge_view)
        ops.merge_batch(ctx, self.mp, self.maps)

    def after(self, k):
        """what the frame's merger would have left in the maps (only where the sequence did not re-enter an old one)"""
        torch = self.torch
        for b in range(3):
            c = self.plant[b][k]
            if c is not None:
                self.maps.coords[b].zero_()
                self.maps.coords[b, : len(c[0]), :3] = torch.from_numpy(c[0]).to(self.dev)
                self.maps.desc[b, : len(c[1])] = torch.from_numpy(c[1]).to(self.dev)
                self.maps.n_points[b] = len(c[0])

    def snapshot(self):
        s, m, g = self.sess, self.maps, self.graphs
        t = dict(pose=s.pose, prev=s.prev, prediction=s.prediction, cur_node=s.cur_node, n_frames=s.n_frames, frame_node=s.frame_node,
                 frame_pose=s.frame_pose, status=s.status, reason=s.reason, n_points=m.n_points, coords=m.coords, desc=m.desc,
                 n_nodes=g.n_nodes, n_edges=g.n_edges, X=g.X, src=g.src, dst=g.dst, Z=g.Z, reentered=self.rb.reentered,
                 reentry_status=self.rb.status, merge_result=self.rb.merge_view.result, archive_status=self.arch.status,
                 n_slots=self.arch.n_slots, archived=self.arch.n_points)
        return {k: v.cpu().numpy().copy() for k, v in t.items()}


def _run_chain(ctx, reentry=True):
    c = Chain(ctx, reentry)
    for k in range(Chain.FRAMES):
        c.upload(k)
        c.launch()
        c.after(k)
        c.log.append(c.snapshot())
    return c


@pytest.fixture(scope="module")
def eager_chain(hip_ctx):
    c = _run_chain(hip_ctx)
    yield c
    c.close()


def test_chain_walks_back_into_its_first_map(hip_ctx, eager_chain):
    c, log = eager_chain, eager_chain.log
    assert [int(s["reason"][0]) for s in log] == [0, 1, 1, 0, 0] and not any(s["status"].any() or s["reentry_status"].any() for s in log)
    assert [s["reentered"].tolist() for s in log] == [[0, 0, 0]] * 2 + [[1, 0, 0]] + [[0, 0, 0]] * 2
    back = log[2]
    assert back["cur_node"][0] == 0 and back["n_nodes"][0] == log[1]["n_nodes"][0] == 2  # the graph gained no node on that frame
    n_merged, n_added, status = back["merge_result"][0].tolist()
    assert status == 0 and n_merged >= 50 and n_added >= Chain.EXTRA and back["archived"][0, 0] == Chain.N
    assert back["n_points"][0] == Chain.N + n_added
    assert back["n_edges"][0] == 2 and (back["src"][0, :2].tolist(), back["dst"][0, :2].tolist()) == ([0, 1], [1, 0])
    assert np.abs(back["pose"][0].reshape(4, 4)[:3, 3] - np.array([0, 0, 0.3])).max() < 1e-3
    assert log[3]["frame_node"][0, :4].tolist() == [0, 0, 1, 0] and log[4]["cur_node"][0] == 0  # the next frame is logged against node 0
    assert log[4]["n_points"][0] == back["n_points"][0] and log[4]["n_nodes"][0] == 2
    trajectory = c.sess.unroll(hip_ctx).cpu().numpy().reshape(3, Chain.FRAMES, 4, 4)
    want = log[4]["X"][0].reshape(-1, 4, 4)[[0, 0, 1, 0, 0]].astype(F) @ log[4]["frame_pose"][0].reshape(-1, 4, 4)
    assert np.abs(trajectory[0] - want).max() < 1e-4
    # the other two sequences equal their run without any re-entry
    plain = _run_chain(hip_ctx, reentry=False)
    for k in range(Chain.FRAMES):
        for key in ("pose", "prev", "prediction", "cur_node", "n_frames", "frame_node", "frame_pose", "status", "reason", "n_points",
                    "coords", "desc", "n_nodes", "n_edges", "X", "src", "dst", "Z"):
            assert log[k][key][1:].tobytes() == plain.log[k][key][1:].tobytes(), (k, key)
    assert log[4]["n_nodes"].tolist() == [2, 4, 1] and plain.log[4]["n_nodes"].tolist() == [3, 4, 1]
    plain.close()


def test_chain_captured_once_and_replayed(hip_ctx, eager_chain):
    import torch
    ctx = hip_ctx
    c = Chain(ctx)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        c.upload(0)
        c.launch()  # warm-up on the capture stream, then back to the state before frame 0
        c.sess.reset()
        c.arch.clear()
        c.bank.clear()
        for t in (c.maps.n_points, c.maps.n_meas, c.sess.frame_node, c.sess.frame_pose, c.rb.reentered, c.rb.status, c.rb.merge_view.result):
            t.zero_()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            c.launch()
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    torch.cuda.synchronize()
    for k in range(Chain.FRAMES):
        c.upload(k)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        c.after(k)
        got, want = c.snapshot(), eager_chain.log[k]
        for key in want:
            assert got[key].tobytes() == want[key].tobytes(), (k, key)
    c.close()


# ---- 7. errors
def test_range_errors_write_the_status_alone(hip_ctx):
    def broken(change):
        rig = Rig(hip_ctx, 2, 4, 24, 4, 6, handover_stride=24, slot_stride=2)
        _walk(rig, np.random.default_rng(70))
        _plant_good(rig, 0)
        _plant_good(rig, 1)
        change(rig)
        before = rig.all_arrays()
        rig.reenter()
        rig.assert_equal()
        after = rig.all_arrays()
        assert rig.out.status.tolist() == [sr.OK, sr.ERR_RANGE] and rig.out.reentered.tolist() == [1, 0]
        for key in after:
            if key not in ("reentry.status", "reentry.reentered"):
                assert after[key][1].tobytes() == before[key][1].tobytes(), key
        rig.close()

    def poke(tensor, array, index, value):
        tensor[index] = value
        array[index] = value

    broken(lambda r: poke(r.graphs.n_nodes, r.w.n_nodes, 1, 5))             # beyond node_stride
    broken(lambda r: poke(r.graphs.n_edges, r.w.n_edges, 1, -1))
    broken(lambda r: poke(r.sess.cur_node, r.w.cur_node, 1, 1))             # m is not the current node
    broken(lambda r: poke(r.graphs.dst, r.w.dst, (1, 1), 0))                # no edge into m
    broken(lambda r: poke(r.graphs.dst, r.w.dst, (1, 0), 2))                # two edges into m
    broken(lambda r: poke(r.arch.n_points, r.a.n_points, (1, 0), 25))       # archived n_points > capacity
    broken(lambda r: poke(r.arch.slot_of_node, r.a.slot_of_node, (1, 0), 2))  # a slot beyond slot_stride
    broken(lambda r: r.d.n_corr.__setitem__(3, r.rb.corr_stride + 1))         # the winner's n_corr beyond corr_stride (pushed with the detector)


def test_call_level_refusals(hip_ctx):
    rig = Rig(hip_ctx, 1, 3, 8, 4, 4, handover_stride=8, slot_stride=2, max_measurements=2)
    lib, ctx = _lib.load(), hip_ctx._h
    sp, rp = ops.session_params(configs.get("kitti")["split"]), ops.reentry_params(configs.REENTRY["kitti"])
    rig.sess.status.fill_(55)
    rig.rb.status.fill_(55)
    D = lambda: (rig.sess.descriptor(), rig.maps.descriptor(), rig.arch.descriptor(), rig.rb.descriptor())  # noqa: E731

    def step(s, m, a):
        return lib.prs_session_step_archive_batch(ctx, C.byref(sp), C.byref(s), C.byref(m) if m is not None else None, C.byref(a) if a is not None else None)

    def reenter(s, m, a, r, p=rp):
        return lib.prs_session_reenter_batch(ctx, C.byref(p), C.byref(s), C.byref(m), C.byref(a), C.byref(r) if r is not None else None)

    s, m, a, r = D()
    assert step(s, None, a) == -1 and step(s, m, None) == -1 and reenter(s, m, a, None) == -1
    for which, field in ((0, "pose"), (1, "state"), (1, "inlier"), (2, "coords"), (2, "slot_of_node"), (2, "poses"), (1, "meas")):
        d = D()
        setattr(d[which], field, None)
        assert step(*d[:3]) == -1, field
        assert reenter(*d) == -1, field
    for field in ("candidates_flat", "result", "corr", "node_of_map", "n_measured", "gate", "merge_corr"):
        d = D()
        setattr(d[3], field, None)
        assert reenter(*d) == -1, field
    for which, field, value in ((2, "capacity", 9), (2, "node_stride", 5), (2, "slot_stride", 0), (2, "max_frames", 3), (1, "batch", 2)):
        d = D()
        setattr(d[which], field, value)
        assert step(*d[:3]) == sr.ERR_RANGE and reenter(*d) == sr.ERR_RANGE, field
    d = D()
    d[3].max_candidates = 0
    assert reenter(*d) == sr.ERR_RANGE
    assert reenter(*D(), p=ops.reentry_params(configs.REENTRY["kitti"], max_translation=-1.0)) == sr.ERR_RANGE
    assert reenter(*D(), p=ops.reentry_params(configs.REENTRY["kitti"], max_translation=float("inf"))) == sr.ERR_RANGE
    for which, field in ((2, "state"), (2, "coords"), (1, "state")):
        d = D()
        setattr(d[which], field, getattr(d[which], field) + 4)
        assert step(*d[:3]) == -5 and reenter(*d) == -5, field
    d = D()
    d[0].handover_stride = 7
    assert step(*d[:3]) == sr.ERR_CAPACITY
    hip_ctx.synchronize()
    assert rig.sess.status[0].item() == 55 and rig.rb.status[0].item() == 55 and rig.sess.n_frames[0].item() == 0
    rig.close()
