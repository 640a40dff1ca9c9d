"""Every back-end entry point inside guard bands (tests/guarded.py) at the buffer sizes and alignments include/proslam_hip.h documents.

The cases run the rigs, builders and restatements of the stages' own GPU tests; guarded.hooked moves every tensor of the ops batches
those build into an arena the moment they are built, at exactly the demanded alignment and with a band of fill bytes on either
side.  Each case runs with fill 0x00 and with fill 0xFF: both runs equal the reference as the stage's own test asserts it, equal
each other byte for byte, and leave every band clean.  B = 3 and the last sequence is the full one: its counts equal the strides, so
its last row adjoins a band.  Memory the library owns (the aligner's job buffers, a place bank's arenas, a prs_map) cannot be
placed from here: tests/test_guard_owned_gpu.py puts it between bands through the library's guard mode (PRS_GUARD_FILL)."""
import numpy as np
import pytest
import torch

import guarded
import point_align_ref as par
import pose_graph_cases as pc
import pose_graph_lm_cases as lc
import session_ref as sr
import test_closure_merge_gpu as closure
import test_merge_dispatch_gpu as merge
import test_pose_algebra_gpu as algebra
import test_place_bank_gpu as bank
import test_point_align_gpu as point_align
import test_pose_graph_gpu as graph
import test_pose_graph_lm_gpu as graph_lm
import test_reentry_gpu as reentry
import test_session_gpu as session
import test_trajectory_gpu as trajectory
import test_world_map_gpu as world_map
import test_world_voxel_gpu as world_voxel
import world_voxel_cases as vc
from srrg2_proslam_amd import _lib, configs, ops
from test_merge_dispatch_gpu import row_ctx  # noqa: F401  (the fixture of the merger's dispatch rows)

pytestmark = pytest.mark.gpu
F = np.float32
B = 3
SESSION = (ops.MapBatch, ops.AlignFrames, ops.PoseGraphBatch, ops.PlaceQueries, ops.PlaceBank, ops.BankDetectorBatch, ops.SessionBatch,
           ops.MapArchive, ops.ReentryBatch, ops.WorldMapBatch)


def lib():
    return _lib.load()


def rows_painted(a, counts, fill):
    """a host array [B, stride, ...] whose rows from counts[b] on are fill bytes: the contract says they are not read"""
    a = a.copy()
    for b, n in enumerate(counts):
        a[b, n:] = guarded.host_fill(a.dtype, fill)
    return a


def rebind(obj):
    """a place bank keeps the address of its caller-owned node_of_map: it is told the new one"""
    if isinstance(obj, ops.PlaceBank):
        assert lib().prs_place_bank_bind_node_of_map(obj._h, obj.node_of_map.data_ptr()) == 0


def numpy_of(**tensors):
    return {k: t.cpu().numpy() for k, t in tensors.items() if t is not None}


# ---- session step (plain and with the archive), re-entry, unroll -------------------------------------------------------------------------
FS, NS, ES, SS = 3, 3, 2, 2   # three frames and two splits: frame FS - 1, node NS - 1, edge ES - 1 and archive slot SS - 1 are the last


def walk(rig, step, rng, cap, fill, archive):
    """frame 0, then two viewpoint splits; the last sequence's map is full at both.  -> nothing: the rig has compared every frame"""
    n_points = np.array([17, 100, cap], np.int32)
    paint = lambda a: rows_painted(a, n_points, fill) if a.shape[:2] == (B, cap) else a  # noqa: E731
    one, none = np.ones(B, np.int32), np.zeros(B, np.int32)
    far = np.tile(reentry.FAR, (B, 1, 1))
    rig.set_handover(0xAB, 7.5, -3, -9)
    for frame in range(FS):
        rig.set_map(coords=paint(rng.normal(size=(B, cap, 4)).astype(F)), desc=paint(rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)),
                    n_points=n_points, n_meas=paint(rng.integers(1, 5, (B, cap)).astype(np.uint32)))
        if archive:
            rig.set_stats(rng, paint, B)
        step(10, 0.25, far, one, none, one)
        rig.assert_equal("frame %d" % frame)
    w = rig.w
    assert w.reason.tolist() == [sr.SPLIT_VIEWPOINT] * B and not w.status.any()
    assert w.n_nodes.tolist() == [NS] * B and w.n_edges.tolist() == [ES] * B and w.n_frames.tolist() == [FS] * B and w.cur_node.tolist() == [NS - 1] * B
    assert w.handover_n_query.tolist() == n_points.tolist()  # handover_stride == capacity: the last sequence fills its slot


def unroll(hip_ctx, rig, arena):
    """n_frames == frame_stride: the last logged frame is the trajectory's last row"""
    arena.paint(rig.sess.trajectory)
    before = np.full((B, FS, 4, 4), guarded.host_fill(F, arena.fill), F)
    want = sr.unroll(rig.w, before)
    got = rig.sess.unroll(hip_ctx).cpu().numpy().reshape(B, FS, 4, 4)
    hip_ctx.synchronize()
    assert got.tobytes() == want.tobytes()
    return got


@pytest.mark.parametrize("cap", [301, 303, 304])
def test_session_step_and_unroll(hip_ctx, cap):
    def case(arena):
        with guarded.hooked(arena, *SESSION):
            rig = session.Rig(B, FS, cap, NS, ES, handover_stride=cap)
        walk(rig, lambda *a: rig.step(hip_ctx, *a), np.random.default_rng([61, cap]), cap, arena.fill, False)
        out = rig.device_arrays()
        out["trajectory"] = unroll(hip_ctx, rig, arena)
        return out

    guarded.both_fills(case)


def archive_case(hip_ctx, cap, history, understate_inlier=False):
    def case(arena):
        with guarded.hooked(arena, *SESSION, after=rebind):
            rig = reentry.Rig(hip_ctx, B, FS, cap, NS, ES, handover_stride=cap, slot_stride=SS, max_measurements=2 if history else 0, max_frames=3)
        if understate_inlier:  # the kernel is given the whole array; the harness believes it one byte shorter
            arena.adopt(rig.arch, "inlier", 1, extent=B * SS * cap - 1, name="archive.inlier.short")
        rng = np.random.default_rng([62, cap, history])
        walk(rig, rig.step, rng, cap, arena.fill, True)
        assert rig.a.n_slots.tolist() == [SS] * B and not rig.a.status.any() and rig.a.n_points[:, SS - 1].tolist() == [17, 100, cap]
        # the last sequence walks back into its first map, which was archived full
        rig.set_map(n_meas=rng.integers(1, 5, (B, cap)).astype(np.uint32))
        reentry._plant_good(rig, B - 1)
        rig.reenter()
        rig.assert_equal("re-entry")
        assert rig.out.reentered.tolist() == [0, 0, 1] and rig.w.cur_node.tolist() == [NS - 1, NS - 1, 0] and rig.w.n_points[B - 1] == cap
        out = rig.all_arrays()
        out["trajectory"] = unroll(hip_ctx, rig, arena)
        rig.close()
        return arena, out

    return case


@pytest.mark.parametrize("history", [False, True], ids=["plain", "history"])
@pytest.mark.parametrize("cap", [301, 303, 304])
def test_archive_step_reentry_and_unroll(hip_ctx, cap, history):
    guarded.both_fills(lambda arena: archive_case(hip_ctx, cap, history)(arena)[1])


def test_an_understated_archive_inlier_extent_is_reported(hip_ctx):
    """the check bites: the archive's last inlier byte, written when the full last sequence's map goes into the last slot, lies
    where the harness believes the trailing band to begin"""
    arena, _ = archive_case(hip_ctx, 303, True, understate_inlier=True)(guarded.Arena(0xFF))
    assert arena.violations() == [("archive.inlier.short", "after", 0)]


# ---- pose bookkeeping: prs_motion_predict_batch, prs_pose_compose_batch --------------------------------------------------------------------
@pytest.mark.parametrize("which", ["predict", "compose"])
def test_pose_algebra_in_arrays_of_exactly_the_batch(oracle, hip_ctx, which):
    """every pose case of the stage's own test in [batch][16] arrays of exactly batch rows, 4-byte aligned"""
    a, b, want = algebra.predict_rows(oracle) if which == "predict" else algebra.compose_rows(oracle)
    op = ops.motion_predict_batch if which == "predict" else ops.pose_compose_batch
    n = len(a)

    def case(arena):
        da, db, out = (arena.take((n, 4, 4), torch.float32, 4, name) for name in ("a", "b", "out"))
        da.copy_(torch.from_numpy(np.ascontiguousarray(a, F)))
        db.copy_(torch.from_numpy(np.ascontiguousarray(b, F)))
        op(hip_ctx, da, db, out)
        hip_ctx.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(algebra._bits(got), algebra._bits(want))
        return dict(out=got)

    guarded.both_fills(case)


# ---- merger and closure merger: the stage tests' own cases that reach capacity and capacity + 1 -----------------------------------------
def maps_of(runs):
    out = {}
    for i, run in enumerate(runs):
        out.update({"%d.%s" % (i, k): v for k, v in numpy_of(**{k: getattr(run.maps, k) for k in merge.ARRAYS + ("n_points", "result")}).items()})
    return out


@pytest.mark.parametrize("row_id", [r for r in merge.ROW_IDS if r != "mono_ekf"])
def test_merger_scene_exactly_full_and_one_more(oracle, row_ctx, row_id):  # noqa: F811
    def case(arena):
        runs = []
        with guarded.hooked(arena, ops.MapBatch, merge.BatchRun, after=lambda o: runs.append(o) if isinstance(o, merge.BatchRun) else None):
            merge.test_scene_exactly_full_and_one_more(oracle, row_ctx, row_id)
        assert runs and all(arena.owns(getattr(r.maps, k)) for r in runs for k in merge.ARRAYS)
        assert all(r.maps.scene_index_map is None or arena.owns(r.maps.scene_index_map) for r in runs)
        return maps_of(runs)

    guarded.both_fills(case)


@pytest.mark.parametrize("row_id", merge.ROW_IDS)
def test_merger_counts_at_the_strides(oracle, row_ctx, row_id):  # noqa: F811
    def case(arena):
        runs = []
        with guarded.hooked(arena, ops.MapBatch, merge.BatchRun, after=lambda o: runs.append(o) if isinstance(o, merge.BatchRun) and o.maps else None):
            merge.test_counts_at_and_beyond_the_strides(oracle, row_ctx, row_id)
        assert runs
        return maps_of(runs)

    guarded.both_fills(case)


@pytest.mark.parametrize("which", ["exactly_full", "errors"])
def test_closure_merger_at_capacity_and_one_more(hip_ctx, which):
    """exactly_full: n_points + n_added == capacity; errors: PRS_ERR_SCENE_FULL among four other pairs of one launch"""
    def case(arena):
        batches = []
        with guarded.hooked(arena, ops.ClosureMergeBatch, after=batches.append):
            if which == "exactly_full":
                closure.test_synthetic_edges((hip_ctx, ops, None), "exactly_full")
            else:
                closure.test_errors_leave_what_the_header_promises((hip_ctx, ops, None))
        mb, = batches
        names = ("coords", "desc", "n_points", "state", "covariance", "n_opt", "inlier", "n_meas", "result")
        assert all(arena.owns(getattr(mb, k)) for k in names if getattr(mb, k) is not None)
        return numpy_of(**{k: getattr(mb, k) for k in names})

    guarded.both_fills(case)


# ---- place bank: query and gather ---------------------------------------------------------------------------------------------------------
def test_place_bank_query_and_gather(hip_ctx):
    """max_candidates 4 of map_stride 5: from the fifth step on the full last sequence finds four candidates, each pair slot holds
    query_stride fixed and query_stride moving rows, the strides of the pair buffers.  The rig's twin databases put
    prs_place_query_batch and prs_place_gather_pairs through the same queries, on guarded memory as well"""
    ctx, maxc, steps = hip_ctx, 4, 5
    base = bank.random_rows(np.random.default_rng(2024), 64)

    def case(arena):
        rng = np.random.default_rng(71)
        with guarded.hooked(arena, ops.PlaceBank, ops.PlaceQueries, ops.PlaceBankLinks, bank.PairBuf, after=rebind):
            rig = bank.Rig(ctx, ops, bank.params(ops, max_candidates=maxc))
        q = rig.q
        hooks = guarded.hooked(arena, ops.PlaceQueries, bank.PairBuf)  # the twins' queries and pair slots: prs_place_query_batch, prs_place_gather_pairs
        hooks.__enter__()
        for s in range(steps):
            items = [bank.item(rng, base, 100 + s, valid_rows=17), bank.item(rng, base, 100 + s, n=100), bank.item(rng, base, 100 + s)]
            rig.upload(items)
            for b, it in enumerate(items):  # rows from n_query to query_stride
                for t in (q.desc, q.xyz, q.valid):
                    arena.paint(t[b, it["n_query"]:])
            rig.launch_query()
            ctx.synchronize()
            res = rig.check_query(items, rig.read(), "step %d" % s)
            rig.launch_append(items)
            ctx.synchronize()
            rig.check_append(items, "step %d" % s)
        hooks.__exit__(None, None, None)
        assert res[B - 1]["candidates"] == [0, 1, 2, 3] and all(len(c) > 0 for c in res[B - 1]["corr"])
        slots = rig.pairs.slots_of(B - 1, maxc)
        assert [(s["n_fixed"], s["n_moving"]) for s in slots] == [(bank.QS, bank.QS)] * maxc
        out = numpy_of(**{k: getattr(q, k) for k in ("match_counts", "best_keys", "candidates", "n_candidates", "corr", "n_corr", "status", "index_query")},
                       **{"pairs." + k: getattr(rig.pairs, k) for k in ("fixed_xyz", "fixed_desc", "moving_xyz", "moving_desc", "n_fixed", "n_moving", "X")},
                       candidates_flat=rig.links.candidates_flat, query_node=rig.links.query_node, node_of_map=rig.bank.node_of_map)
        rig.close()
        return out

    guarded.both_fills(case, nbytes=64 << 20)


# ---- point aligner -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [65, 257])
def test_point_aligner_counts_at_the_strides(hip_ctx, stride):
    """the last pair has stride points in both clouds and stride correspondences"""
    rng = np.random.default_rng([81, stride])
    P = ops.point_align_params(configs.get("kitti")["loop"], min_num_correspondences=0)
    items = [point_align.synthetic(rng, n) + (point_align.GUESS,) for n in (3, 40, stride)]
    want = [par.align(point_align.checker_params(P), it[3], it[0], it[1], it[2]) for it in items]

    def case(arena):
        batches = []

        def slack(pb):  # upload writes the first rows of every array; the rest is not read
            for t in (pb.fixed, pb.moving, pb.corr, pb.inlier_mask):
                arena.paint(t)
            batches.append(pb)

        with guarded.hooked(arena, ops.PointAlignBatch, after=slack):
            got = point_align.run_batch(hip_ctx, ops, P, items, stride)
        for it, (X, res, mask), w in zip(items, got, want):
            point_align.assert_same(X, res, mask, *w, what=len(it[2]))
        pb, = batches
        assert pb.fixed_stride == pb.moving_stride == pb.corr_stride == stride and pb.n_corr.tolist()[-1] == stride
        return numpy_of(X=pb.X, result=pb.result, inlier_mask=pb.inlier_mask)

    guarded.both_fills(case)


# ---- pose graph: Gauss-Newton and Levenberg-Marquardt ---------------------------------------------------------------------------------------
def graph_case(hip_ctx, mod, cs, P, wants, **strides):
    lm = mod is graph_lm

    def case(arena):
        batches = []

        def slack(g):  # upload writes the rows of the graph's nodes and edges; the rest, and the workspace, holds nothing
            for t in (g.X, g.fixed, g.src, g.dst, g.Z, g.omega, g.workspace):
                arena.paint(t)
            batches.append(g)

        with guarded.hooked(arena, ops.PoseGraphBatch, after=slack):
            g = mod.run_batch(hip_ctx, ops, cs, P, **strides)
        size = lib().prs_pose_graph_lm_workspace_bytes if lm else lib().prs_pose_graph_workspace_bytes
        assert g is batches[0] and g.workspace.numel() * 8 == g.workspace_bytes == size(len(cs), g.node_stride, g.envelope_blocks)
        for b, (c, w) in enumerate(zip(cs, wants)):
            mod.assert_same(g.poses_of(b), g.lm_result_of(b) if lm else g.result_of(b), w, "%s at %d" % (c["name"], b))
        return numpy_of(X=g.X, result=g.lm_result if lm else g.result)

    return case


@pytest.mark.parametrize("solver", ["gn", "lm"])
def test_pose_graph_three_rings_at_their_strides(hip_ctx, solver):
    """ring8 has 8 nodes, 8 edges and an envelope of 21 blocks: nothing is left over in any array or in the workspace"""
    ring = pc.case("ring8")
    if solver == "gn":
        damping, form, eps = graph.VARIANTS[0]
        mod, P, w = graph, graph.params(ops, damping, form, eps), graph.want(ring, damping, form, eps)
    else:
        mod, P, w = graph_lm, graph_lm.params(ops), graph_lm.want(ring)
    assert w["envelope_blocks"] == 21 and len(ring["poses"]) == 8 and len(ring["src"]) == 8
    guarded.both_fills(graph_case(hip_ctx, mod, [ring] * B, P, [w] * B, node_stride=8, edge_stride=8, envelope_blocks=21))


@pytest.mark.parametrize("solver", ["gn", "lm"])
def test_pose_graph_wide_row_in_the_workspace(hip_ctx, solver):
    """200 nodes with the closure (0, 199) at node_stride 1024: the row is factorised in place in a workspace of exactly the envelope"""
    c = lc.wide_row()
    if solver == "gn":
        damping, form, eps = graph.VARIANTS[0]
        mod, P, w = graph, graph.params(ops, damping, form, eps, iterations=2), graph.want(c, damping, form, eps, iterations=2)
    else:
        mod, P, w = graph_lm, graph_lm.params(ops, rounds=2), graph_lm.want(c, rounds=2)
    guarded.both_fills(graph_case(hip_ctx, mod, [c], P, [w], node_stride=1024, envelope_blocks=w["envelope_blocks"]))


def test_pose_graph_append_closures_from_the_detector(hip_ctx):
    """the stage's own chain -- prs_place_query_batch, prs_place_gather_pairs, the matcher, the loop aligner,
    prs_pose_graph_append_closures and the optimiser -- with the detector's and the graphs' arrays in the arena"""
    def case(arena):
        graphs = []
        with guarded.hooked(arena, ops.PoseGraphBatch, ops.LoopDetectorBatch, after=lambda o: graphs.append(o) if isinstance(o, ops.PoseGraphBatch) else None):
            graph.test_closures_from_the_detector((hip_ctx, ops))
        assert graphs and all(arena.owns(g.X) and arena.owns(g.Z) for g in graphs)
        return {"%d.%s" % (i, k): getattr(g, k).cpu().numpy() for i, g in enumerate(graphs) for k in ("X", "src", "dst", "Z", "n_edges", "append_status")}

    guarded.both_fills(case, nbytes=128 << 20)


# ---- world map ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [0, 1], ids=["exact", "one_short"])
def test_world_map(hip_ctx, monkeypatch, short):
    """out_stride == the last sequence's total (and one less: PRS_ERR_CAPACITY, the last written row adjoins the band)"""
    p = ops.world_map_params(min_n_opt=1)
    rp = world_map.ref.params(min_n_opt=1, require_inlier=False, include_live=True, refresh_state=False)

    def seqs_for(fill):
        seqs = world_map._batch(65, 5, B)
        for s in seqs:  # rows from n_points on, in the live map and in every slot
            for name in ("coords", "desc", "n_opt", "inlier", "state"):
                s["live"][name][s["live"]["n_points"]:] = guarded.host_fill(s["live"][name].dtype, fill)
                for slot, n in enumerate(s["slots"]["n_points"]):
                    s["slots"][name][slot, n:] = guarded.host_fill(s["slots"][name].dtype, fill)
        return seqs

    total = world_map.ref.world_map(seqs_for(0)[-1], rp, None)["n_total"]
    assert total > 130

    def case(arena):
        monkeypatch.setattr(world_map, "SENTINEL", arena.fill)
        with guarded.hooked(arena, *SESSION):
            rig = world_map.Rig(hip_ctx, seqs_for(arena.fill), total - short)
            assert rig.wm.workspace.numel() == lib().prs_world_map_workspace_bytes(B, 5, 65) and arena.owns(rig.wm.workspace)
            arena.paint(rig.wm.workspace)
            want = rig.check(p, what="guarded")
            assert (want[-1]["n_total"], want[-1]["n_out"], want[-1]["status"]) == (total, total - short, world_map.ref.PRS_ERR_CAPACITY if short else 0)
            first = rig.outputs()
            rig.check(ops.world_map_params(min_n_opt=1, refresh_state=True), what="guarded, refreshed")
        return dict(first, **{"refreshed." + k: v for k, v in rig.outputs().items()})

    guarded.both_fills(case)


# ---- world voxel --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [0, 1], ids=["exact", "one_short"])
def test_world_voxel(hip_ctx, monkeypatch, short):
    """in_stride == the last cloud's rows, a table of exactly its 64 voxels (every slot taken), out_stride == n_voxels and one less;
    both positions; the workspace for exactly this table"""
    n, voxels = (100, 200, 257), (30, 50, 64)

    def clouds_for(fill):
        clouds = [vc.make_cloud(world_voxel._rng(91, b), n[-1], n[b], world_voxel.SIZE, voxels[b]) for b in range(B)]
        for c in clouds:
            for k in ("xyz",) + world_voxel.INPUTS:
                c[k][c["n"]:] = guarded.host_fill(c[k].dtype, fill)
        return clouds

    def case(arena):
        monkeypatch.setattr(world_voxel, "SENTINEL", arena.fill)
        with guarded.hooked(arena, ops.WorldVoxelBatch):
            rig = world_voxel.Rig(hip_ctx, clouds_for(arena.fill), voxels[-1] - short, table_stride=64)
        for k in sorted(rig.dev):
            arena.adopt(rig.dev, k, 16 if k in ("xyz", "desc") else 4, name="in_" + k)
        assert rig.vx.workspace.numel() == lib().prs_world_voxel_workspace_bytes(B, n[-1], 64) and arena.owns(rig.vx.workspace)
        assert rig.vx.workspace.numel() < lib().prs_world_voxel_workspace_bytes(B, n[-1], 1024)  # not the table ops.py would pick
        arena.paint(rig.vx.workspace)
        out = {}
        for want, position in zip(rig.check_both(world_voxel.SIZE, "guarded"), world_voxel.POSITIONS):
            assert (want[-1]["n_voxels"], want[-1]["n_out"]) == (64, 64 - short)
            assert want[-1]["status"] == (world_voxel.ref.PRS_ERR_CAPACITY if short else 0) and want[0]["n_out"] == 30
            out.update({position + "." + k: v for k, v in rig.outputs().items()})
        return out

    guarded.both_fills(case)


# ---- trajectory evaluator -----------------------------------------------------------------------------------------------------------------
def drive(n):
    """n ground-truth poses [n, 4, 4] float64: 0.8 m a frame along a slowly turning road"""
    k = np.arange(n)
    heading = 0.6 * np.sin(k / 300.0) + k / 2500.0
    step = 0.8 * np.stack([np.sin(heading), 0.02 * np.sin(k / 40.0), np.cos(heading)], axis=1)
    G = np.tile(np.eye(4), (n, 1, 1))
    G[:, :3, 3] = np.cumsum(step, axis=0) - step[0]
    c, s = np.cos(heading), np.sin(heading)
    G[:, 0, 0], G[:, 0, 2], G[:, 2, 0], G[:, 2, 2] = c, s, -s, c
    return G


@pytest.mark.parametrize("n", [3, 257, 4801, 6401])
def test_trajectory_at_frame_stride(hip_ctx, n):
    """frame_stride == n in the last sequence: staged clouds and distances (<= 4800 rows), staged clouds alone (<= 6400), nothing
    staged; the cumulative distances reach the workspace's last element; valid mask and frame_error on"""
    G = drive(n)
    est = trajectory.drifted(G, n)
    counts = (min(3, n), max(n // 2, 3), n)
    mask = (np.random.default_rng(n).random(n) < 0.9).astype(np.uint8)  # of the middle sequence; the full one has every row valid

    def seqs_for(fill):
        seqs = []
        for b, k in enumerate(counts):
            e, g = (np.full((n, 16), guarded.host_fill(F, fill), F) for _ in range(2))
            e[:k], g[:k] = est[:k], trajectory.rows16(G[:k])
            v = np.full(n, fill, np.uint8)
            v[:k] = mask[:k] if b == 1 else 1
            seqs.append((e, g, k, v))
        return seqs

    wants = [trajectory.ref_of(s) for s in seqs_for(0)]
    assert all(w["status"] == 0 and w["kitti_margin"] >= 1e-6 for w in wants)  # no subsequence end within rounding of a length

    def case(arena):
        with guarded.hooked(arena, ops.TrajectoryEvalBatch, aligns={"result": 8}):  # prs_trajectory_result holds doubles
            batch = trajectory.Batch(seqs_for(arena.fill), n, with_valid=True)
        res, ferr, work = batch.run(hip_ctx, ops.trajectory_params())
        for b, seq in enumerate(batch.seqs):
            trajectory.check(res[b], ferr[b], wants[b], trajectory.cloud_scale(seq), "n %d seq %d" % (n, b))
            assert np.all(work[b, counts[b]:] == trajectory.SENTINEL) and (b == 1 or work[b, counts[b] - 1] > 0)
        return dict(result=batch.ev.result.cpu().numpy(), frame_error=ferr, workspace=work)

    guarded.both_fills(case)
