"""Every kernel instantiation merge_batch_launch (csrc/mapping.hip) can launch -- the seven merge_kernel instantiations,
smoother_kernel and smoother_tail_kernel -- off the world frame, in batches, at its capacity and LDS edges and with faulty maps
inside a batch.  Each launch merges one frame into B DIFFERENT maps (tests/merge_cases.py: sizes, seeds, poses and local-map
origins differ, measurement_in_scene != measurement_in_world) and every map is compared with the per-map CPU checker bit for bit
(all map arrays, the pose table, the result triple); the rows of DISPATCH are also compared with the float64 restatement of
tests/mapping_ref.py, with the constants of tests/test_mapping_ref.py.  tests/test_merge_dispatch_table.py keeps DISPATCH and the
library's variant table and plan (prs_merge_plan) in step.

The tail kernel: the checker's test-only trace (oracle.binding_mapping.smoother_trace) tells which landmarks are still iterating,
without a repeated state, after kTailRounds * 8 = 24 iterations; those are certain to be handed to smoother_tail_kernel.  With the
"far" cases (depths of 20..150 m) about 7 % of the optimised landmarks are, so a map of 1500 points keeps more than
kTailPerFrame = 64 of them after round three and its hand-over is deferred to a later round (test_tail_hand_over_is_deferred).

Nothing here provokes a GPU fault: every "fault" is a status code of a kernel that returns normally."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import binding as ob
from oracle import binding_mapping as om
from srrg2_proslam_amd import _lib, ops
from tests import mapping_ref as mr
from tests import merge_cases as mc
from tests.test_mapping_ref import assert_within

pytestmark = pytest.mark.gpu

def MG(args):
    """merge_kernel<EST, DIM, PHASE> as a kernel trace prints it (EST 0 = weighted mean, 1 = EKF, 2 = pose-based smoother)"""
    return "void prs::merge_kernel<%s>(prs::MergeArgs)" % args


# one row per instantiation merge_batch_launch can launch, with the knobs that select it (merge / smoother: the kernels by the
# names a kernel trace prints).  index_map: the row's launches go through scene_index_map and corr_from_aligner = 1 (one row
# per estimator; the depth form has tests/test_mapping_gpu.py)
DISPATCH = [
    {"id": "weighted_mean", "kind": "weighted_mean", "fused": False, "index_map": True, "merge": [MG("0, 4, 0")], "smoother": []},
    {"id": "smoother_fused", "kind": "smoother", "fused": True, "index_map": False, "merge": [MG("2, 4, 0")], "smoother": []},
    {"id": "smoother_split", "kind": "smoother", "fused": False, "index_map": True, "merge": [MG("2, 4, 1"), MG("2, 4, 2")],
     "smoother": ["prs::smoother_kernel(prs::MergeArgs)", "prs::smoother_tail_kernel(prs::MergeArgs)"]},
    {"id": "stereo_ekf", "kind": "stereo_ekf", "fused": False, "index_map": True, "merge": [MG("1, 4, 0")], "smoother": []},
    {"id": "depth_ekf", "kind": "depth_ekf", "fused": False, "index_map": False, "merge": [MG("1, 3, 0")], "smoother": []},
    {"id": "mono_ekf", "kind": "mono_ekf", "fused": False, "index_map": False, "merge": [MG("1, 2, 0")], "smoother": []},
]
ROW = {r["id"]: r for r in DISPATCH}


def row_kernels(row):
    """the row's launches in order: one merge_kernel, or front | smoother_kernel | smoother_tail_kernel | back"""
    return row["merge"][:1] + row["smoother"] + row["merge"][1:]
ROW_IDS = [r["id"] for r in DISPATCH]
SMOOTHER_ROWS = ["smoother_fused", "smoother_split"]

ERR_CAPACITY, ERR_RANGE, ERR_UNSUPPORTED = -2, -4, -5
STATUS_OF_CHECKER = {-1: ERR_RANGE, om.ERR_DUPLICATE: om.ERR_DUPLICATE, om.ERR_HISTORY: om.ERR_HISTORY, om.ERR_SCENE_FULL: om.ERR_SCENE_FULL}
ARRAYS = ("coords", "desc", "state", "covariance", "n_opt", "inlier", "n_meas", "meas")


@pytest.fixture
def row_ctx(request, monkeypatch, hip_ctx):
    """-> context_for(row): the session context, or a fresh one created under PRS_MERGE_FUSED=1 (the knob is read at creation)"""
    made = []

    def context_for(row):
        if not row["fused"]:
            return hip_ctx
        monkeypatch.setenv("PRS_MERGE_FUSED", "1")
        made.append(ops.Context(0))
        return made[-1]

    yield context_for
    for c in made:
        c.close()


def gpu_params(po):
    assert C.sizeof(_lib.MergerParams) == C.sizeof(om.MergerParams)
    pg = _lib.MergerParams()
    C.memmove(C.byref(pg), C.byref(po), C.sizeof(_lib.MergerParams))
    return pg


def bits(a):
    """float32 bit patterns, every NaN the same value (as tests/test_mapping_gpu.py::_assert_map_equal)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


class BatchRun:
    """B maps on the device next to B checker maps.  step() merges one frame into every map on both sides and compares all of them.
    ctx = None runs the checker side only (the cases can be tried without a GPU)."""

    def __init__(self, ctx, P, seqs, capacity, max_frames=None, measurement_stride=512, corr_stride=1024, index_map=False, max_meas=None):
        self.ctx, self.P, self.pg, self.seqs, self.B = ctx, P, gpu_params(P), seqs, len(seqs)
        self.capacity, self.index_map = capacity, index_map
        self.max_meas = seqs[0].max_meas if max_meas is None else max_meas
        self.max_frames = max_frames or max(s.n_frames for s in seqs)
        self.mstride, self.cstride = measurement_stride, corr_stride
        for s in seqs:
            s.max_meas = self.max_meas
        self.ref = [s.new_map(capacity) for s in seqs]
        self.poses = [om.pose_table(self.max_frames) for _ in seqs]
        self.dead = [False] * self.B      # maps whose arrays are no longer defined (an estimator / capacity fault half way)
        self.frames_done = [0] * self.B
        self.tail_certain = []            # per step: per map the landmarks certain to reach the tail kernel
        self.dev = mr.Deviations()
        self.maps = None
        if ctx is not None:
            self.maps = ops.MapBatch(0, self.B, capacity, self.max_meas, self.max_frames, measurement_stride, corr_stride)
            self.maps.corr_from_aligner = 1 if index_map else 0
            if index_map:
                self.maps.scene_index_map = torch.zeros((self.B, capacity), dtype=torch.int32, device="cuda")
            self.upload_maps()

    # ---- device side ---------------------------------------------------------------------------------------------------
    def stacked(self, name):
        return np.stack([getattr(m, name) for m in self.ref])

    def upload_maps(self):
        mp, t = self.maps, lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        mp.coords.copy_(t(self.stacked("coords")))
        mp.desc.copy_(t(self.stacked("desc")))
        mp.state.copy_(t(self.stacked("state")))
        mp.covariance.copy_(t(self.stacked("covariance")))
        mp.n_opt.copy_(t(self.stacked("n_opt").view(np.int32)))
        mp.inlier.copy_(t(self.stacked("inlier")))
        mp.n_meas.copy_(t(self.stacked("n_meas").view(np.int32)))
        mp.meas.copy_(t(self.stacked("meas").view(np.int32).reshape(self.B, self.capacity, -1, 7)))
        mp.poses.copy_(t(np.stack(self.poses).view(np.float32).reshape(self.B, self.max_frames, 24)))
        mp.n_points.copy_(t(np.array([m.n_points for m in self.ref], np.int32)))

    def upload_frame(self, inputs, slots):
        B, mp = self.B, self.maps
        z4 = np.zeros((B, self.mstride, 4), np.float32)
        zd = np.zeros((B, self.mstride, 32), np.uint8)
        cr = np.zeros((B, self.cstride, 3), np.int32)
        nm, nc = np.zeros(B, np.int32), np.zeros(B, np.int32)
        Tw, Ts = np.zeros((B, 4, 4), np.float32), np.zeros((B, 4, 4), np.float32)
        im = np.zeros((B, self.capacity), np.int32)
        for b, (tw, ts, z, desc, corr, imap) in enumerate(inputs):
            n = len(z)
            z4[b, :n, : z.shape[1]], zd[b, :n], nm[b], nc[b], Tw[b], Ts[b] = z, desc, n, len(corr), tw, ts
            first, second = ("moving_idx", "fixed_idx") if self.index_map else ("fixed_idx", "moving_idx")  # the aligner's orientation
            cr[b, : len(corr), 0], cr[b, : len(corr), 1], cr[b, : len(corr), 2] = corr[first], corr[second], corr["response"].view(np.int32)
            if imap is not None:
                im[b, : len(imap)] = imap
        t = lambda a: torch.from_numpy(a).cuda()
        mp.measurement.copy_(t(z4))
        mp.measurement_desc.copy_(t(zd))
        mp.corr.copy_(t(cr))
        mp.n_measured.copy_(t(nm))
        mp.n_corr.copy_(t(nc))
        mp.measurement_in_world.copy_(t(Tw))
        mp.measurement_in_scene.copy_(t(Ts))
        mp.frame.copy_(t(np.asarray(slots, np.int32)))
        if self.index_map:
            mp.scene_index_map.copy_(t(im))

    def download(self):
        mp = self.maps
        d = {n: getattr(mp, n).cpu().numpy() for n in ARRAYS + ("poses", "n_points", "result")}
        d["n_opt"], d["n_meas"] = d["n_opt"].view(np.uint32), d["n_meas"].view(np.uint32)
        return d

    def assert_map(self, d, b, m, poses, n_frames, what):
        n = m.n_points
        assert int(d["n_points"][b]) == n, (what, b, "n_points", int(d["n_points"][b]), n)
        for name in ("coords", "state"):
            assert np.array_equal(bits(d[name][b, :n, :3]), bits(getattr(m, name)[:n, :3])), (what, b, name)
        assert np.array_equal(bits(d["covariance"][b, :n]), bits(m.covariance[:n])), (what, b, "covariance")
        for name in ("desc", "n_opt", "inlier", "n_meas"):
            assert np.array_equal(d[name][b, :n], getattr(m, name)[:n]), (what, b, name)
        if m.max_measurements > 0:
            used = np.arange(m.meas.shape[1])[None, :] < m.n_meas[:n, None]
            g, o = d["meas"][b, :n], m.meas[:n].view(np.int32).reshape(n, m.meas.shape[1], 7)
            assert np.array_equal(g[used], o[used]), (what, b, "history")
        assert np.array_equal(bits(d["poses"][b, :n_frames]), bits(poses[:n_frames].view(np.float32).reshape(n_frames, 24))), (what, b, "pose table")

    def device_map(self, d, b):
        """map b of the device as an om.Map (for the float64 checks)"""
        m = om.Map(self.capacity, self.max_meas)
        m.n_points = int(d["n_points"][b])
        for name in ("coords", "desc", "state", "covariance", "n_opt", "inlier", "n_meas"):
            getattr(m, name)[...] = d[name][b]
        m.meas[...] = np.ascontiguousarray(d["meas"][b]).view(om.MEAS_DTYPE).reshape(m.meas.shape)
        return m

    # ---- one frame ---------------------------------------------------------------------------------------------------------
    def step(self, k, mutate=None, slots=None, f64=False, what=""):
        """frame k of every sequence; mutate(b, corr, n_points) -> corr may spoil a map's correspondences.
        -> per map the checker's return code"""
        slots = [k] * self.B if slots is None else slots
        inputs, befores, rcs, results, tails = [], [], [], [], []
        for b, seq in enumerate(self.seqs):
            m = self.ref[b]
            if self.dead[b] or k >= seq.n_frames:
                Tw = np.eye(4, dtype=np.float32)
                inputs.append((Tw, Tw, np.zeros((0, seq.dim), np.float32), np.zeros((0, 32), np.uint8), np.zeros(0, ob.CORR_DTYPE), None))
                befores.append(None)
                rcs.append(None)
                results.append(None)
                tails.append(0)
                continue
            Tw, Ts, z, desc, corr = seq.inputs(k, m, self.cstride)
            assert len(z) <= self.mstride
            if mutate is not None:
                corr = mutate(b, corr, m.n_points)
            imap, ocorr = None, corr
            if self.index_map:  # correspondences name clipped indices j; scene_index_map[j] is the landmark
                imap = np.zeros(max(len(corr), 1), np.int32)
                imap[: len(corr)] = corr["fixed_idx"]
                ocorr = corr.copy()
                ocorr["fixed_idx"] = np.arange(len(corr))
            before = m.copy()
            with om.smoother_trace(self.capacity) as tr:
                rc, res = om.merge(self.P, Tw, Ts, self.poses[b], slots[b], m, z, desc, ocorr, imap if self.index_map else None)
            tails.append(int(((tr.iterations > 24) & ((tr.first_repeat < 0) | (tr.first_repeat > 24))).sum()))
            inputs.append((Tw, Ts, z, desc, ocorr, imap))
            befores.append(before)
            rcs.append(rc)
            results.append((res.n_merged, res.n_added, res.flags))
        self.tail_certain.append(tails)
        d = None
        if self.ctx is not None:
            self.upload_frame(inputs, slots)
            ops.merge_batch(self.ctx, self.pg, self.maps)
            self.ctx.synchronize()
            d = self.download()
        for b in range(self.B):
            if rcs[b] is None:
                continue
            tag = "%s frame %d" % (what, k)
            if rcs[b] == 0:
                self.frames_done[b] = max(self.frames_done[b], slots[b] + 1)
                if d is not None:
                    assert tuple(int(v) for v in d["result"][b]) == results[b], (tag, b, d["result"][b], results[b])
                    self.assert_map(d, b, self.ref[b], self.poses[b], self.frames_done[b], tag)
                if f64:
                    after = self.device_map(d, b) if d is not None else self.ref[b]
                    Tw, Ts, z, desc, ocorr, imap = inputs[b]
                    mr.check_frame(self.P, befores[b], after, self.poses[b], slots[b], Tw, Ts, z, desc, ocorr, scene_index_map=imap if self.index_map else None,
                                   dev=self.dev)
                continue
            status = STATUS_OF_CHECKER[rcs[b]]
            if d is not None:
                assert int(d["result"][b, 2]) == status, (tag, b, "status", d["result"][b], status)
            if status in (ERR_RANGE, om.ERR_DUPLICATE):
                # a refused correspondence vector: the device leaves the map as it was (the sequential checker has updated the
                # landmarks in front of the fault; it continues from the state before the frame)
                self.ref[b] = befores[b]
                if d is not None:
                    assert int(d["result"][b, 0]) == 0 and int(d["result"][b, 1]) == 0
                    self.assert_map(d, b, befores[b], self.poses[b], self.frames_done[b], tag + " (refused)")
            else:
                self.dead[b] = True
        return rcs

    def run(self, n_frames, **kw):
        out = []
        for k in range(n_frames):
            out.append(self.step(k, **kw))
        return out

    def assert_untouched(self, what):
        """every live map still equals its checker map (after a launch that must not have changed anything)"""
        d = self.download()
        for b in range(self.B):
            if not self.dead[b]:
                self.assert_map(d, b, self.ref[b], self.poses[b], self.frames_done[b], what)


def small_batch(kind, n_maps, n_frames=4, seed=500, n_world=(24, 56), **kw):
    rng = np.random.default_rng(seed)
    return [mc.Sequence(kind, seed + b, int(rng.integers(*n_world)), n_frames, no_corr=(n_maps > 4 and b == 1), empty_frame=(1 if (n_maps > 4 and b == 3) else None), **kw)
            for b in range(n_maps)]


# ---- the dispatch rows: six distinct maps per launch, off the world frame, against the checker and against float64 -------------
@pytest.mark.parametrize("binning", [0, 1])
@pytest.mark.parametrize("row_id", ROW_IDS)
def test_row_merges_distinct_maps_off_the_world_frame(oracle, row_ctx, row_id, binning):
    row = ROW[row_id]
    run = BatchRun(row_ctx(row), mc.merger_params(row["kind"], binning), mc.distinct_batch(row["kind"]), capacity=1600, index_map=row["index_map"])
    # what the library plans for these inputs on this context (host only)
    assert ops.merge_plan(run.pg, run.maps.descriptor(), ops.dispatch_env(run.ctx))["kernels"] == row_kernels(row)
    rcs = run.run(5, f64=True, what=row_id)
    assert all(rc == 0 for step in rcs for rc in step)
    assert_within(run.dev, "%s binning %d" % (row_id, binning))
    assert run.dev.checked > 300 and (run.dev.added > 300 or row["kind"] == "mono_ekf")
    for b, m in enumerate(run.ref):  # the scene frame is not the world frame
        assert np.abs(m.coords[: m.n_points, :3] - m.state[: m.n_points, :3]).max() > 10.0, b


# ---- batch size ------------------------------------------------------------------------------------------------------------------
def cu_count():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("row_id", ROW_IDS)
def test_batch_sizes(oracle, row_ctx, row_id):
    """1, 2 and one more map than the device has CUs, every map compared"""
    row = ROW[row_id]
    ctx = row_ctx(row)
    for n_maps in (1, 2, cu_count() + 1):
        run = BatchRun(ctx, mc.merger_params(row["kind"], 1), small_batch(row["kind"], n_maps), capacity=256, measurement_stride=64, corr_stride=256,
                       index_map=row["index_map"])
        rcs = run.run(4, what="%s B=%d" % (row_id, n_maps))
        assert all(rc == 0 for step in rcs for rc in step)


def test_more_maps_than_tail_waves(oracle, hip_ctx):
    """2049 maps through the split smoother: smoother_tail_kernel's grid stops at 2048 waves and its grid-stride loop starts; the
    stragglers of all maps share one list, and each is handed back to its own map's pose table, carry and descriptor row"""
    n_maps = 2049
    seqs = small_batch("smoother", n_maps, n_frames=5, seed=9000, far=True, response_max=50, n_world=(16, 40))
    run = BatchRun(hip_ctx, mc.merger_params("smoother", 0, target_merges=0), seqs, capacity=192, measurement_stride=48, corr_stride=192)
    rcs = run.run(5, what="B=2049")
    assert all(rc == 0 for step in rcs for rc in step)
    assert_tail_used(run, min_landmarks=4000)  # measured on the CPU: 9746 landmarks in 2000 of the 2049 maps, at most 9 in one frame of one map


def assert_tail_used(run, min_landmarks, min_maps=2):
    per_map = np.array(run.tail_certain).sum(axis=0)
    print("landmarks certain to reach the tail kernel: %d in %d maps, at most %d in one frame of one map" % (
        per_map.sum(), (per_map > 0).sum(), np.array(run.tail_certain).max()))
    assert (per_map > 0).sum() >= min_maps and per_map.sum() >= min_landmarks, (per_map.sum(), (per_map > 0).sum())


def test_tail_hand_over_is_deferred(oracle, hip_ctx):
    """one map keeps more than kTailPerFrame = 64 iterating landmarks after round three (its hand-over waits for a later round) next
    to small maps that hand over at once"""
    seqs = [mc.Sequence("smoother", 5, 1500, 6, far=True, response_max=50)] + small_batch("smoother", 3, n_frames=6, seed=77, far=True, response_max=50, n_world=(100, 200))
    P = mc.merger_params("smoother", 0, target_merges=0, estimator={"chi2_delta": 1e-7})
    run = BatchRun(hip_ctx, P, seqs, capacity=1600, measurement_stride=1536, corr_stride=1600, max_meas=8)
    rcs = run.run(6, what="deferred tail")
    assert all(rc == 0 for step in rcs for rc in step)
    big = [t[0] for t in run.tail_certain]
    print("map 0, landmarks past 24 iterations per frame:", big)
    assert max(big) > 64, big  # measured on the CPU: 50, 65, 90, 100 in frames 2..5
    assert_tail_used(run, min_landmarks=200)  # measured on the CPU: 398 in 4 maps


# ---- capacities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", [r for r in ROW_IDS if r != "mono_ekf"])
def test_scene_exactly_full_and_one_more(oracle, row_ctx, row_id):
    """n_points + n_added == capacity fits; one landmark more is PRS_ERR_SCENE_FULL.  The capacity is no multiple of 32 and the
    next frame references the last landmark (the last word of the `seen` bitmap); max_frames - 1 is the last pose row, max_frames
    PRS_ERR_RANGE; the measurement stride is exactly the larger of the two frames"""
    row = ROW[row_id]
    kind = row["kind"]
    P = mc.merger_params(kind, 0, target_merges=0)
    probe = mc.Sequence(kind, 41, 150, 2)
    m = probe.new_map(400)
    Tw, Ts, z, desc, corr = probe.inputs(0, m)
    assert om.merge(P, Tw, Ts, om.pose_table(2), 0, m, z, desc, corr)[0] == 0
    cap = m.n_points
    assert cap % 32 != 0 and cap > 64
    seqs = [mc.Sequence(kind, 41, 150, 2), mc.Sequence(kind, 41, 150, 2), mc.Sequence(kind, 43, 60, 2)]
    n1 = len(seqs[0].frames[1]["z"])
    run = BatchRun(row_ctx(row), P, seqs, capacity=cap, max_frames=2, measurement_stride=max(n1, len(z)), corr_stride=cap, index_map=row["index_map"])
    # map 1 holds one landmark already: the same frame needs cap + 1 rows
    run.ref[1].add_landmark((0, 0, 1), (0, 0, 1), np.eye(3), desc=np.full(32, 255, np.uint8))
    if run.maps is not None:
        run.upload_maps()
    rcs = run.step(0, what=row_id)
    assert rcs == [0, om.ERR_SCENE_FULL, 0] and run.ref[0].n_points == cap
    # frame 1 (pose row max_frames - 1): every landmark seen again, the last one among them
    seen_last = []

    def note(b, corr, n_points):
        seen_last.append(bool((corr["fixed_idx"] == n_points - 1).any()))
        return corr
    rcs = run.step(1, mutate=note, what=row_id)
    assert rcs[0] == 0 and rcs[2] == 0
    if not seen_last[0]:
        pytest.fail("case does not reference the last landmark")
    if run.maps is not None:  # the pose table is full: frame == max_frames is refused, nothing changes
        run.maps.frame.fill_(2)
        ops.merge_batch(run.ctx, run.pg, run.maps)
        run.ctx.synchronize()
        assert run.maps.result[:, 2].cpu().tolist() == [ERR_RANGE] * 3
        run.assert_untouched(row_id + " frame == max_frames")


@pytest.mark.parametrize("row_id", ROW_IDS)
def test_counts_at_and_beyond_the_strides(oracle, row_ctx, row_id):
    """n_measured == measurement_stride and n_corr == corr_stride are served; one more of either is PRS_ERR_CAPACITY and a negative
    count PRS_ERR_RANGE for that map alone, its arrays untouched"""
    row = ROW[row_id]
    kind = row["kind"]
    seqs = [mc.Sequence(kind, 300 + b, 120, 3, response_max=50) for b in range(6)]
    ms = max(len(f["z"]) for s in seqs for f in s.frames)
    P = mc.merger_params(kind, 0, target_merges=0)
    # corr_stride: the largest correspondence count of the run (found with the checker alone)
    dry = BatchRun(None, P, [mc.Sequence(kind, 300 + b, 120, 3, response_max=50) for b in range(6)], capacity=256, measurement_stride=ms)
    dry.run(2)
    cs = max(len(s.inputs(2, m)[4]) for s, m in zip(dry.seqs, dry.ref))
    run = BatchRun(row_ctx(row), P, seqs, capacity=256, measurement_stride=ms, corr_stride=cs, index_map=row["index_map"])
    rcs = run.run(3, what=row_id)
    assert all(rc == 0 for step in rcs for rc in step)
    mp = run.maps
    assert int(mp.n_corr.max()) == cs  # (ms is the largest frame of the run by construction)
    # the same frame again with spoilt counts in maps 1, 2, 4, 5: nothing may change there; maps 0 and 3 are refused too
    # (their history / estimate would move), so give them an empty frame
    nm, nc = mp.n_measured.cpu().numpy().copy(), mp.n_corr.cpu().numpy().copy()
    nm[[0, 3]], nc[[0, 3]] = 0, 0
    nm[1], nc[2], nm[4], nc[5] = ms + 1, cs + 1, -1, -3
    mp.n_measured.copy_(torch.from_numpy(nm).cuda())
    mp.n_corr.copy_(torch.from_numpy(nc).cuda())
    ops.merge_batch(run.ctx, run.pg, mp)
    run.ctx.synchronize()
    st = mp.result.cpu().numpy()
    assert st[:, 2].tolist() == [0, ERR_CAPACITY, ERR_CAPACITY, 0, ERR_RANGE, ERR_RANGE], st
    assert (st[[1, 2, 4, 5], :2] == 0).all()
    run.assert_untouched(row_id + " counts beyond the strides")


@pytest.mark.parametrize("row_id", SMOOTHER_ROWS)
def test_history_exactly_full_then_one_more(oracle, row_ctx, row_id):
    """max_measurements = 4: the landmark's first measurement and three updates fill the history exactly; the fifth is PRS_ERR_HISTORY
    for the maps that reach it, while the map without correspondences and the late map go on"""
    row = ROW[row_id]
    seqs = [mc.Sequence("smoother", 60, 80, 6, response_max=50), mc.Sequence("smoother", 61, 90, 6, no_corr=True), mc.Sequence("smoother", 62, 70, 6, response_max=50),
            mc.Sequence("smoother", 63, 60, 6, empty_frame=0, response_max=50)]  # map 3 starts one frame later
    run = BatchRun(row_ctx(row), mc.merger_params("smoother", 0, target_merges=0), seqs, capacity=700, max_meas=4, index_map=row["index_map"])
    rcs = run.run(4, what=row_id)
    assert all(rc == 0 for step in rcs for rc in step)
    assert run.ref[0].n_meas.max() == 4 and run.ref[2].n_meas.max() == 4 and run.ref[3].n_meas.max() == 3
    assert run.step(4, what=row_id) == [om.ERR_HISTORY, 0, om.ERR_HISTORY, 0]
    assert run.step(5, what=row_id) == [None, 0, None, om.ERR_HISTORY]


@pytest.mark.parametrize("row_id", SMOOTHER_ROWS)
def test_pose_cache_carries_the_lds_request_past_64k(oracle, row_ctx, row_id):
    """max_frames = 800: 800 x 84 B of pose cache with a small bin table; frames land in the first and the last rows"""
    row = ROW[row_id]
    seqs = [mc.Sequence("smoother", 80 + b, 60 + 20 * b, 4, response_max=50) for b in range(3)]
    P = mc.merger_params("smoother", 1, target_merges=0, row_bins=4, col_bins=6)
    run = BatchRun(row_ctx(row), P, seqs, capacity=256, max_frames=800, measurement_stride=128, corr_stride=256)
    for k, slot in enumerate((0, 1, 798, 799)):
        assert run.step(k, slots=[slot] * 3, what=row_id) == [0, 0, 0]
    assert run.ref[0].n_opt.max() >= 3


# ---- LDS request -----------------------------------------------------------------------------------------------------------------
def lds_request(row, capacity, max_frames, row_bins, col_bins):
    """the dynamic LDS merge_batch_launch asks for (csrc/mapping.hip: off_owner .. off_pose_cache)"""
    a16 = lambda v: (v + 15) & ~15
    nbins = (row_bins + 2) * (col_bins + 2)
    shared = 4 * 16 * 4 + 5 * 4  # MergeShared: four 4x4 float matrices, five ints
    pose = max_frames * 21 * 4 if row["kind"] == "smoother" else 0
    return a16(nbins * 4) * 2 + a16(nbins * 8) + a16((capacity + 31) // 32 * 4) + a16(shared) + a16(4 * 4) + a16(pose)


@pytest.mark.parametrize("row_id", ROW_IDS)
def test_lds_request_under_over_64k_largest_and_first_refused(oracle, row_ctx, row_id):
    """per kernel symbol (the hipFuncSetAttribute branch is per symbol): a bin grid under 64 KiB of dynamic LDS, one over it, the
    largest request that is accepted and the first that is refused (PRS_ERR_UNSUPPORTED, nothing launched, maps untouched)"""
    row = ROW[row_id]
    kind = row["kind"]
    cam = mc.camera(kind)
    ctx = row_ctx(row)
    cap, frames, limit = 256, 4, 160 * 1024

    def widest(rb):
        return max(c for c in range(1, 4096) if lds_request(row, cap, frames, rb, c) <= limit)
    # the fewest row bins whose widest accepted grid AND the next one still have columns of at least one pixel
    rb = min(r for r in range(2, 64) if widest(r) + 1 <= cam["cols"])
    c_max = widest(rb)
    assert lds_request(row, cap, frames, rb, c_max) <= limit < lds_request(row, cap, frames, rb, c_max + 1)
    assert lds_request(row, cap, frames, 20, 60) < 64 * 1024 < lds_request(row, cap, frames, 60, 80) < limit
    for r, c in ((20, 60), (60, 80), (rb, c_max)):
        seqs = [mc.Sequence(kind, 700 + b, 100 + 30 * b, frames, response_max=50) for b in range(3)]
        run = BatchRun(ctx, mc.merger_params(kind, 1, row_bins=r, col_bins=c, target_merges=0), seqs, capacity=cap, max_frames=frames, measurement_stride=256,
                       corr_stride=256, index_map=row["index_map"])
        rcs = run.run(frames, what="%s grid %dx%d" % (row_id, r, c))
        assert all(rc == 0 for step in rcs for rc in step)
    run.pg = gpu_params(mc.merger_params(kind, 1, row_bins=rb, col_bins=c_max + 1, target_merges=0))
    run.maps.result.fill_(77)
    with pytest.raises(_lib.ProslamHipError) as e:
        ops.merge_batch(ctx, run.pg, run.maps)
    assert e.value.status == ERR_UNSUPPORTED
    ctx.synchronize()
    assert (run.maps.result.cpu().numpy() == 77).all()
    run.assert_untouched(row_id + " refused LDS request")


@pytest.mark.parametrize("row_id", ROW_IDS)
def test_bin_width_of_one_pixel_and_just_below(oracle, row_ctx, row_id):
    """as many row bins as the canvas has rows (376 for KITTI) are exactly 1 pixel wide and served (378 x 6 bins fit the LDS; a grid
    that fine in the columns too would not); one more is refused (merger_projective_impl.cpp:35-47 throws)"""
    row = ROW[row_id]
    kind = row["kind"]
    rows = mc.camera(kind)["rows"]
    seqs = [mc.Sequence(kind, 900 + b, 150, 4, response_max=50) for b in range(3)]
    run = BatchRun(row_ctx(row), mc.merger_params(kind, 1, row_bins=rows, col_bins=4), seqs, capacity=700, index_map=row["index_map"])
    rcs = run.run(4, what=row_id)
    assert all(rc == 0 for step in rcs for rc in step)
    run.pg = gpu_params(mc.merger_params(kind, 1, row_bins=rows + 1, col_bins=4))
    with pytest.raises(_lib.ProslamHipError) as e:
        ops.merge_batch(run.ctx, run.pg, run.maps)
    assert e.value.status == ERR_UNSUPPORTED
    run.assert_untouched(row_id + " bin width below one pixel")


# ---- faults inside a batch ---------------------------------------------------------------------------------------------------------
def spoil(kind_of_fault):
    def mutate(b, corr, n_points):
        corr = corr.copy()
        if len(corr) < 8:
            return corr
        if b == 1 and kind_of_fault == "range":
            corr["fixed_idx"][len(corr) // 2] = n_points  # one past the last landmark
        if b == 1 and kind_of_fault == "negative":
            corr["fixed_idx"][3] = -1
        if b == 1 and kind_of_fault == "measurement":
            corr["moving_idx"][5] = 10 ** 6
        if b == 1 and kind_of_fault == "duplicate":
            corr["fixed_idx"][len(corr) - 1] = corr["fixed_idx"][2]
        return corr
    return mutate


@pytest.mark.parametrize("fault", ["range", "negative", "measurement", "duplicate"])
@pytest.mark.parametrize("row_id", ROW_IDS)
def test_faulty_vector_inside_a_batch(oracle, row_ctx, row_id, fault):
    """map 1's correspondence vector is refused with the checker's code in frame 2 (rows with an index map meet the bad landmark
    index through it: scene_index_map[j] is one past the last landmark, or negative);
    its arrays stay as they were, its neighbours equal the checker in that frame and in the healthy frame after it -- and so does
    map 1 itself"""
    row = ROW[row_id]
    kind = row["kind"]
    seqs = [mc.Sequence(kind, 1200 + b, 90 + 25 * b, 4, response_max=50) for b in range(4)]
    run = BatchRun(row_ctx(row), mc.merger_params(kind, 0, target_merges=0), seqs, capacity=512, index_map=row["index_map"])
    assert run.run(2, what=row_id) == [[0] * 4] * 2
    want = om.ERR_DUPLICATE if fault == "duplicate" else -1
    assert run.step(2, mutate=spoil(fault), what="%s %s" % (row_id, fault)) == [0, want, 0, 0]
    assert run.step(3, what=row_id + " after the fault") == [0, 0, 0, 0]


@pytest.mark.parametrize("order", ["duplicate_first", "range_first"])
@pytest.mark.parametrize("row_id", ["weighted_mean", "smoother_fused", "smoother_split", "stereo_ekf"])
def test_first_fault_in_vector_order_is_reported(oracle, row_ctx, row_id, order):
    """one vector holding a duplicate and an out-of-range entry, on 64 maps of one launch: every map reports the checker's fault,
    the first one in vector order"""
    row = ROW[row_id]
    kind = row["kind"]
    seqs = [mc.Sequence(kind, 1300, 500, 3, response_max=50) for _ in range(64)]
    run = BatchRun(row_ctx(row), mc.merger_params(kind, 0, target_merges=0), seqs, capacity=640, index_map=row["index_map"])
    assert run.run(2, what=row_id) == [[0] * 64] * 2

    def mutate(b, corr, n_points):
        corr = corr.copy()
        n = len(corr)
        assert n > 300  # the two faults sit in different waves of the correspondence loop
        dup, rng_at = (10, n - 7) if order == "duplicate_first" else (n - 7, 10)
        corr["fixed_idx"][dup] = corr["fixed_idx"][dup - 5]
        corr["fixed_idx"][rng_at] = n_points + 3
        return corr
    want = om.ERR_DUPLICATE if order == "duplicate_first" else -1
    assert run.step(2, mutate=mutate, what="%s %s" % (row_id, order)) == [want] * 64


@pytest.mark.parametrize("row_id", [r for r in ROW_IDS if r != "mono_ekf"])  # (the mono form adds no points)
def test_scene_full_inside_a_batch(oracle, row_ctx, row_id):
    """map 2 runs out of rows in frame 1 (PRS_ERR_SCENE_FULL); its neighbours equal the checker in that frame and the next"""
    row = ROW[row_id]
    kind = row["kind"]
    sizes = [60, 80, 400, 70]
    seqs = [mc.Sequence(kind, 1400 + b, sizes[b], 3, response_max=50) for b in range(4)]
    run = BatchRun(row_ctx(row), mc.merger_params(kind, 0), seqs, capacity=420, index_map=row["index_map"])
    assert run.step(0, what=row_id) == [0, 0, 0, 0]
    assert run.step(1, what=row_id) == [0, 0, om.ERR_SCENE_FULL, 0]
    assert run.step(2, what=row_id) == [0, 0, None, 0]
