"""The library's OWN device and pinned memory between guard bands: the context's work, staging and pinned arenas, the aligner's six
job buffers, the arrays of a prs_map, a prs_pcf handle's blocks, a place database's and a place bank's arrays.  tests/guarded.py
puts the arrays a caller hands over between bands; this file does the same for what the caller never sees, through the library's
guard mode (include/proslam_hip.h, "guard mode"): a context created under PRS_GUARD_FILL=00 or ff allocates every block
as [front band | user bytes | tail band] with the tail band at the first byte behind the bytes the host formula asked for, paints
the user bytes with the fill -- the reused arenas and job buffers again at every request -- and checks the bands before a block is
freed and whenever ops.Context.guard_check() is asked.

Every case runs under fill 00, then under ff, on a fresh context for each (the knob is read at creation):
  - it asserts what the stage's own test asserts against its oracle or restatement, through that test's rig, rows and references;
  - the outputs of the two runs are byte-identical (guarded.same_bytes): a word the library reads before it writes it is 0 in
    the one and -1 / NaN in the other;
  - guard_check() == 0 at the end, blocks freed by growth included, and the context closes without a latched violation;
  - the regions the case is about were reached (guard_regions(); the names are printed, run with -s to see them).
The host-pointer entry points have the default path as their reference, as tests/test_staging_reuse_gpu.py has: the same call on a
context without guard mode, byte for byte.

What this cannot see: several arrays carved from ONE block stay invisible to each other -- the selective extractor's work block
(mask, candidates, selection), the brute-force matcher's bitmaps and accumulators, the merger's tail block, the sections of a
staging block.  A write past one of them into the next lands in user bytes.  Only the 0x00 / 0xFF comparison can notice it."""
import ctypes as C

import numpy as np
import pytest
import torch

import closure_merge_cases as cc
import guarded
import place_cases as plc
import pose_graph_cases as pc
import scene_clip_cases as scc
import test_align_dispatch_gpu as dispatch
import test_bruteforce_dispatch_gpu as bfd
import test_closure_merge_gpu as closure
import test_closure_merge_sizes_gpu as closure_sizes
import test_extractor_edges_gpu as edges
import test_finder_aligner_gpu as finder
import test_guard_tracking_gpu as tracking
import test_merge_dispatch_gpu as merge
import test_place_bank_gpu as bank
import test_pose_graph_gpu as graph
import test_pose_graph_lm_gpu as graph_lm
import test_scene_clip_edges_gpu as clip
import test_staging_reuse_gpu as staging
from helpers import corr_equal, make_align_case
from oracle import binding_mapping as om
from srrg2_proslam_amd import _lib, configs, ops, synthetic as syn
from test_guard_tracking_gpu import one_oracle_frame, one_oracle_run  # noqa: F401  (the rigs' oracles answer once per frame / image)
from tests import merge_cases as mc

pytestmark = pytest.mark.gpu
F = np.float32
ARENAS_WORK = ["arena.work0", "arena.work1", "arena.work2", "arena.work3"]
JOB = ["align.ctl", "align.ops", "align.lattice", "align.rowcache", "align.qcache", "align.missq"]


# ---- the harness -----------------------------------------------------------------------------------------------------------------
def guarded_context(monkeypatch, fill, **knobs):
    """a fresh context in guard mode with this fill; knobs: the other environment variables it reads at creation.  The variable is
    taken back at once: a context a rig creates for itself is not in guard mode unless the case makes it so"""
    with monkeypatch.context() as m:
        m.setenv("PRS_GUARD_FILL", "%02x" % fill)
        for name in ("PRS_NO_LONE_GN", "PRS_FUSED_ALIGN", "PRS_NO_PREFILTER", "PRS_MERGE_FUSED"):
            if knobs.get(name):
                m.setenv(name, "1")
            else:
                m.delenv(name, raising=False)
        ctx = ops.Context(0)
    ctx.use_torch_stream()
    return ctx


def names_of(ctx):
    return sorted({r["name"] for r in ctx.guard_regions()})


def note(ctx, what):
    """the regions of a case while its handles live (finish() sees the context after they have gone)"""
    print("guard regions [%s]: %s" % (what, " ".join(names_of(ctx))))


def finish(ctx, what, reached=()):
    """zero violations, the regions the case is about, and a context that goes without a latched violation"""
    seen = names_of(ctx)
    print("guard regions [%s]: %s" % (what, " ".join(seen)))
    n, lines = ctx.guard_check(report=True)
    assert n == 0 and lines == [], (what, lines)
    assert set(reached) <= set(seen), (what, sorted(set(reached) - set(seen)))
    ctx.close()
    assert ctx.close_status == 0, what


def under_both_fills(monkeypatch, what, run, reached=(), **knobs):
    """run(ctx, fill) -> dict of numpy arrays, on a fresh guarded context per fill: 00 first, then ff"""
    outs = []
    for fill in guarded.FILLS:
        ctx = guarded_context(monkeypatch, fill, **knobs)
        try:
            outs.append(run(ctx, fill))
            finish(ctx, "%s, fill %02x" % (what, fill), reached)
        finally:
            ctx.close()
    guarded.same_bytes(*outs)
    return outs


def as_arrays(x, prefix="out"):
    """any nesting of dicts, sequences, ctypes structs, numbers, bytes and arrays as a flat dict of numpy arrays (for same_bytes)"""
    if isinstance(x, dict):
        return {k2: v for k in sorted(x, key=str) for k2, v in as_arrays(x[k], "%s.%s" % (prefix, k)).items()}
    if isinstance(x, (tuple, list)):
        return {k2: v for i, item in enumerate(x) for k2, v in as_arrays(item, "%s.%d" % (prefix, i)).items()}
    if isinstance(x, C.Structure):
        return {prefix: np.frombuffer(bytes(x), np.uint8)}
    if isinstance(x, (bytes, bytearray)):
        return {prefix: np.frombuffer(bytes(x), np.uint8)}
    if x is None:
        return {prefix: np.zeros(0, np.uint8)}
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return {prefix: np.ascontiguousarray(np.asarray(x))}


class Borrowed:
    """a context a rig believes to own: everything but close()"""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def close(self):
        pass


def test_the_entry_points_refuse_a_context_without_guard_mode(hip_ctx):
    with pytest.raises(ops.ProslamHipError) as e:
        hip_ctx.guard_check()
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(ops.ProslamHipError) as e:
        hip_ctx.guard_regions()
    assert e.value.status == _lib.ERR_UNSUPPORTED


# ---- 1. the aligner's job buffers ------------------------------------------------------------------------------------------------
# rows of the dispatch table that carve the six buffers differently; lone8_plain is the one with the query cache and its miss queue
# (a lattice finder with four survivor slots: prs::align_plan's `reuse`)
ALIGN_ROWS = ("lone4_plain", "lone8_plain", "tp4_mprior", "five_mprior", "depth4", "generic8", "fused_by_size")


def job_buffers_of(row):
    """the job buffers a row's plan asks for, from the row's knobs (csrc/align.hip, align_batch_launch)"""
    if row.get("gn") is None or row["max_fixed"] > 1024:
        return []  # the fused kernel owns nothing
    kdtree = row.get("fkw", {}).get("search_type", 2) == 0
    reuse = not kdtree and dispatch.SLOT_WIDTHS.get(row["max_fixed"], 4) == 4
    return JOB[:3] + ([] if kdtree else JOB[3:4]) + (JOB[4:] if reuse else [])


def knobs_of(row):
    return dict(PRS_NO_LONE_GN=row.get("no_lone", 0), PRS_FUSED_ALIGN=row.get("fused", 0))


def frames_of(frames):
    return {k: getattr(frames, k).cpu().numpy() for k in tracking.OUTPUTS}


def parity_run(oracle, monkeypatch, row, cases, cfg):
    """run(ctx, fill): the row's batch through the dispatch test's own comparison (oracle bits, float64 fixed point)"""
    def run(ctx, fill):
        made, real = [], dispatch._run_batch
        with monkeypatch.context() as m:
            m.setattr(dispatch, "_run_batch", lambda *a, **kw: made.append(real(*a, **kw)) or made[-1])
            n_corr, converged = dispatch._row_parity(oracle, ctx, row, cases, cfg)
        assert max(n_corr) > 100 and converged >= 1, (n_corr, converged)
        return frames_of(made[0])
    return run


@pytest.mark.parametrize("row_id", ALIGN_ROWS)
def test_aligner_rows(oracle, monkeypatch, one_oracle_frame, row_id):  # noqa: F811
    row = tracking.ROW[row_id]
    cfg, cases = tracking.row_cases(oracle, row)
    under_both_fills(monkeypatch, "aligner " + row_id, parity_run(oracle, monkeypatch, row, cases, cfg), job_buffers_of(row), **knobs_of(row))
    assert len(one_oracle_frame) == len(cases)


def test_the_aligner_rows_reach_all_six_buffers():
    assert {n for r in ALIGN_ROWS for n in job_buffers_of(tracking.ROW[r])} == set(JOB)
    assert job_buffers_of(tracking.ROW["tp4_mprior"]) == JOB[:3] and job_buffers_of(tracking.ROW["lone4_plain"]) == JOB[:4]
    assert job_buffers_of(tracking.ROW["fused_by_size"]) == []


@pytest.mark.parametrize("max_fixed", [512, 513, 1024, 1025])
def test_aligner_max_fixed_edges_with_a_full_frame(oracle, monkeypatch, one_oracle_frame, max_fixed):  # noqa: F811
    """the slot change (512 / 513) and the last split batch (1024; 1025 runs the fused kernel), one frame cut to exactly max_fixed"""
    cfg, cases = dispatch._cases("kitti", 9100 + max_fixed, 3, max_fixed, full=1)
    for c in cases:
        c["scale"] = oracle.info_scale_from_nopt(c["n_opt"])
    assert len(cases[0]["fixed"]) == max_fixed
    row = dict(id="max_fixed %d" % max_fixed, max_fixed=max_fixed)
    reached = JOB[:4] if max_fixed <= 1024 else []
    under_both_fills(monkeypatch, row["id"], parity_run(oracle, monkeypatch, row, cases, cfg), reached)


@pytest.mark.parametrize("max_fixed", [2047, 2048])
def test_aligner_max_fixed_beyond_the_limits_is_refused_with_nothing_allocated(monkeypatch, max_fixed):
    """2047 is beyond the fused kernel's LDS, 2048 the class code's unit: refused before any launch, as the dispatch test asserts"""
    cfg, cases = dispatch._cases("kitti", 9300, 1, max_fixed, full=1)
    c = cases[0]
    assert len(c["fixed"]) == max_fixed

    def run(ctx, fill):
        frames = ops.AlignFrames(0, 1, max_fixed, len(c["xyz"]))
        frames.upload(0, c["fixed"], c["dfix"], c["xyz"], None, c["dmov"], c["X0"])
        fp, ap = dispatch._device_params(cfg, {}, {})
        with pytest.raises(ops.ProslamHipError) as ei:
            ops.align_batch(ctx, fp, ap, frames)
        assert ei.value.status == _lib.ERR_UNSUPPORTED
        assert not set(names_of(ctx)) & set(JOB)
        return dict(n_corr=frames.n_corr.cpu().numpy())

    under_both_fills(monkeypatch, "max_fixed %d" % max_fixed, run)


@pytest.mark.parametrize("row_id", ALIGN_ROWS)
def test_aligner_batch_of_2_then_6_then_2_on_one_context(monkeypatch, row_id):
    """the growth frees blocks that were checked, the shrink runs on used blocks painted again: every result equals the same batch on
    a fresh context, byte for byte"""
    row = tracking.ROW[row_id]
    cfg, cases = dispatch._cases(row["cfg"], 7100 + 13 * dispatch.DISPATCH.index(row), dispatch.FRAMES_PER_ROW, row["max_fixed"], full=1)
    for c in cases:
        c["scale"] = ops.info_scale_from_nopt(c["n_opt"])
    fkw, akw, mprior = row.get("fkw", {}), row.get("akw", {}), bool(row.get("mprior"))

    def batch(ctx, n):
        return frames_of(dispatch._run_batch(ctx, cfg, cases[:n], row["max_fixed"], fkw, akw, False, mprior, expect=dispatch.row_kernels(row)))

    def run(ctx, fill):
        fresh = {}
        for n in (2, 6):
            other = guarded_context(monkeypatch, fill, **knobs_of(row))
            try:
                fresh[n] = batch(other, n)
                finish(other, "aligner %s fresh batch of %d, fill %02x" % (row_id, n, fill), job_buffers_of(row))
            finally:
                other.close()
        out = {}
        for step, n in enumerate((2, 6, 2)):
            got = batch(ctx, n)
            for k in got:
                assert got[k].tobytes() == fresh[n][k].tobytes(), (row_id, "batch %d of %d" % (step, n), k)
            out.update({"%d.%s" % (step, k): v for k, v in got.items()})
        return out

    under_both_fills(monkeypatch, "aligner %s 2-6-2" % row_id, run, job_buffers_of(row), **knobs_of(row))


# ---- 2. the work arenas ----------------------------------------------------------------------------------------------------------
def stage_bruteforce(row_id):
    r = {r["id"]: r for r in bfd.DISPATCH}[row_id]

    def stage(ctx, fill, oracle, monkeypatch):
        made, real = [], bfd._upload

        def borrowed(case, mp):
            for name in ("PRS_BF_GLOBAL_STATE", bfd.TWO):  # (read per launch: prs::dispatch_env)
                if name in case.env:
                    mp.setenv(name, case.env[name])
                else:
                    mp.delenv(name, raising=False)
            ctx.set_bruteforce_dense_phase(case.mode)
            return Borrowed(ctx)

        with monkeypatch.context() as m:
            m.setattr(bfd, "_context", borrowed)
            m.setattr(bfd, "_upload", lambda case: made.append(real(case)) or made[-1])
            bfd.test_dispatch_row(oracle, m, r)
        clouds, = made
        return as_arrays(dict(n=clouds.n_matches, status=clouds.status), "bf." + row_id)  # (rows of `matches` behind n_matches are the caller's)

    return stage


def stage_extractor(ctx, fill, oracle, monkeypatch):
    images = tracking.fast_images()
    po, pg = edges.fast_params(15, 1, 10 ** 5, (2, 3), False)
    counts = tracking.fast_counts(po, images)
    arena = guarded.Arena(fill)
    out = tracking.features_of(arena, tracking.run_fast(arena, ctx, pg, images, counts[-1], 0))
    edges.check_fast(po, images, out)
    arena.check()
    return tracking.as_dict(out, "fast.")


def stage_selective(ctx, fill, oracle, monkeypatch):
    images, proj, radius, masks, pad, refs, counts = tracking.sel_case("tracking")
    arena = guarded.Arena(fill)
    out = tracking.features_of(arena, tracking.run_sel(arena, ctx, edges.sel_params(tracking.SEL_TARGET, tracking.SEL_WIDTH), images, counts[-1],
                                                       pad, proj, radius, masks))
    edges.check_sel(out, refs)
    arena.check()
    return tracking.as_dict(out, "sel.")


def stage_merger(ctx, fill, oracle, monkeypatch):
    """the smoother row this context was created for: fused under PRS_MERGE_FUSED=1, else front | smoother | back"""
    row = merge.ROW["smoother_fused" if ops.dispatch_env(ctx).merge_fused else "smoother_split"]
    run = merge.BatchRun(ctx, mc.merger_params(row["kind"], 1), mc.distinct_batch(row["kind"]), capacity=1600, index_map=row["index_map"])
    assert ops.merge_plan(run.pg, run.maps.descriptor(), ops.dispatch_env(ctx))["kernels"] == merge.row_kernels(row)
    rcs = run.run(3, what=row["id"])
    assert all(rc == 0 for step in rcs for rc in step)
    d = run.download()
    n = d["n_points"]
    return {"merge." + k: np.concatenate([d[k][b, :n[b]].reshape(-1) for b in range(run.B)]) for k in ("coords", "state", "covariance", "desc", "n_opt")}


def stage_clipper(ctx, fill, oracle, monkeypatch):
    """three scenes of three tiles through count + scatter (the tile counts are the work block), with the age table"""
    batch = scc.small(2049)
    assert clip.shape_of(3, 2049) == "count+scatter"
    out = clip.launch(ctx, clip.load(batch, True), batch)
    clip.check(out, batch, True)
    return as_arrays(out, "clip")


STAGES = dict(bf_popcount=stage_bruteforce("popcount_fused_1024"), bf_mfma=stage_bruteforce("mfma_flush"),
              bf_two_workgroups=stage_bruteforce("fused_matrix_512_switch_on"), extractor=stage_extractor, selective=stage_selective,
              merger=stage_merger, clipper=stage_clipper)
ORDERS = {
    "fused_merger": ("bf_popcount", "extractor", "merger", "selective", "bf_mfma", "clipper", "bf_two_workgroups"),
    "split_merger": ("clipper", "bf_two_workgroups", "selective", "merger", "extractor", "bf_mfma", "bf_popcount"),
}


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_work_arenas_back_to_back_on_one_context(oracle, monkeypatch, one_oracle_run, order):  # noqa: F811
    """every user of ARENA_WORK_0..3 in turn on one context, each against its own reference: a stage finds the arenas the one before it
    left, painted again.  The merger's fused / split choice is read when the context is created, so each order has one of them"""
    def run(ctx, fill):
        out = {}
        for name in ORDERS[order]:
            out.update(STAGES[name](ctx, fill, oracle, monkeypatch))
            damaged, lines = ctx.guard_check(report=True)
            assert damaged == 0, (name, lines)
        return out

    under_both_fills(monkeypatch, "work arenas, " + order, run, ARENAS_WORK + ["info_lut"], PRS_MERGE_FUSED=order == "fused_merger")


# ---- 3. staging: every host-pointer entry point built on prs::Staging ------------------------------------------------------------
KITTI, ICL = staging.KITTI, staging.ICL
E2, D0 = np.zeros((0, 2), F), np.zeros((0, 32), np.uint8)


def _flat_image():
    return np.full((96, 160), 128, np.uint8)


def _bruteforce_relaunch():
    """four prototypes for 96 + 96 rows: more candidates than the 16 a descriptor the first launch has room for"""
    import bruteforce_cases as bc
    import bruteforce_ref as br
    rng = staging._rng(20)
    df, dm = bc.shared_prototypes(rng, 4, 96, 96, 4)
    assert np.count_nonzero(br.hamming_all(df, dm) < 30) > 16 * 96
    bp = ops.bruteforce_params(30.0, 0.9)
    return lambda ctx: ops.bruteforce_match(ctx, bp, df, dm)


def _closure(name):
    c = cc.edge(name)
    return lambda ctx: ops.closure_merge(ctx, closure.params_of(c["P"]), c["scene"], c["measurement"], c["measurement_desc"], c["corr"],
                                         c["transform"], c.get("scene_in_world"), c.get("transform_is_scene_in_measurement", 0),
                                         c.get("corr_from_aligner", 0))


def _graph(name, lm):
    c = pc.case(name)
    if lm:
        P = graph_lm.params(ops)
        return lambda ctx: ops.pose_graph_optimize_lm(ctx, P, c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], c["omega"])
    P = graph.params(ops, *graph.VARIANTS[0])
    return lambda ctx: ops.pose_graph_optimize(ctx, P, c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], c["omega"])


def _empty_place():
    query = syn.random_descriptors(staging._rng(21), 64)
    pp = ops.place_params(KITTI["place"], max_candidates=2, minimum_age_difference_to_candidates=0)

    def run(ctx):
        db = ops.PlaceDatabase(ctx)
        out = db.query(pp, 0, query)
        db.close()
        return out
    return run


def _empty_depth():
    frames, _ = syn.rgbd_image_sequence(staging._rng(7), ICL, 1)
    depth = np.ascontiguousarray(frames[0][1][:64, :96])
    return lambda ctx: ops.depth_measurements(ctx, ops.depth_params("u16", 0.001), depth, E2, D0, np.zeros(0, F))


def _empty_point_align():
    pp = ops.point_align_params(KITTI["loop"])
    return lambda ctx: ops.point_align(ctx, pp, np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros((0, 2), np.int64), np.eye(4, dtype=F))


# entry point -> the calls of one case: the smallest its own test has (tests/test_staging_reuse_gpu.py's small calls, the pose-graph
# and closure-merger cases by name) and an empty input where the entry point has one
STAGING = {
    "prs_stereo_match": lambda: [staging._stereo(64), lambda ctx: ops.stereo_match(
        ctx, ops.stereo_params(KITTI["stereo_matcher"], KITTI["camera"]["rows"]), E2, D0, E2, D0)],
    "prs_triangulate": lambda: [staging._triangulate(64), lambda ctx: ops.triangulate(ctx, ops.triangulator_params(KITTI), np.zeros((0, 4), F))],
    "prs_scene_clip": lambda: [staging._scene_clip(200), lambda ctx: ops.scene_clip(
        ctx, ops.projector_params(KITTI), np.eye(4, dtype=F), staging.I4, np.zeros((0, 4), F), D0)],
    "prs_bruteforce_match": lambda: [staging._bruteforce(96), _bruteforce_relaunch(), lambda ctx: ops.bruteforce_match(ctx, ops.bruteforce_params(), D0, D0)],
    "prs_selection_order": lambda: [staging._selection_order(96), lambda ctx: ops.selection_order(ctx, np.zeros(0, np.uint8))],
    "prs_extract_features": lambda: [staging._extract(96, 160, 512), lambda ctx: ops.extract_features(
        ctx, ops.extractor_params(15, 1, 500, 3, 3, ops.SELECT_LIBSTDCXX, 32768), _flat_image(), capacity=512)],
    "prs_extract_features_selective": lambda: [staging._selective(96, 160, 0, 512), lambda ctx: ops.extract_features_selective(
        ctx, ops.selective_extractor_params("GFTT", "ORB-256", 100, 10, max_candidates=16384), _flat_image(), radius=10, capacity=512)],
    "prs_gn_step": lambda: [staging._gn_step(0)],
    "prs_selftest_reciprocal": lambda: [lambda ctx: ops.selftest_reciprocal(ctx)],
    "prs_depth_measurements": lambda: [staging._depth(64, 96, 48), _empty_depth()],
    "prs_point_align": lambda: [staging._point_align(48), _empty_point_align()],
    "prs_closure_merge": lambda: [_closure("no_stats"), _closure("n_corr_0")],
    "prs_place_query": lambda: [staging._place(64), _empty_place()],
    "prs_pose_graph_optimize": lambda: [_graph("ring8", False), _graph("n65", False), _graph("n1", False)],
    "prs_pose_graph_optimize_lm": lambda: [_graph("ring8", True), _graph("n1", True)],
}
STAGE_ARENA = {"prs_bruteforce_match": "arena.stage_bruteforce", "prs_gn_step": "arena.stage_solver", "prs_selftest_reciprocal": "arena.stage_solver",
               "prs_pose_graph_optimize": "arena.stage_pose_graph", "prs_pose_graph_optimize_lm": "arena.stage_pose_graph"}
_default_path = {}


def answer(f, ctx):
    """the call's result, or the status it was refused with"""
    try:
        return as_arrays(f(ctx))
    except ops.ProslamHipError as e:
        return dict(refused=np.array([e.status], np.int32))


def default_path(name):
    """[(call, its answer on a fresh context without guard mode)], once for both fills"""
    if name not in _default_path:
        calls, plain = STAGING[name](), ops.Context(0)
        try:
            _default_path[name] = [(f, answer(f, plain)) for f in calls]
        finally:
            plain.close()
    return _default_path[name]


@pytest.mark.parametrize("name", sorted(STAGING))
def test_staging_entry_point(monkeypatch, name):
    """the device block and its pinned mirror both carry bands; the mirror's are checked on the host"""
    def run(ctx, fill):
        out = {}
        for i, (f, want) in enumerate(default_path(name)):
            got = answer(f, ctx)
            assert sorted(got) == sorted(want), (name, i)
            for k in want:
                assert got[k].tobytes() == want[k].tobytes(), (name, "call %d" % i, k)
            out.update({"%d.%s" % (i, k): v for k, v in got.items()})
        pinned = [r for r in ctx.guard_regions() if r["pinned"]]
        assert [r["name"] for r in pinned] == ["arena.pinned"]
        return out

    under_both_fills(monkeypatch, name, run, [STAGE_ARENA.get(name, "arena.stage"), "arena.pinned"])


def test_the_staging_cases_are_the_entry_points_built_on_the_helper():
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    named = set()
    for f in (f for f in os.listdir(csrc) if f.endswith(".hip")):
        named |= set(re.findall(r'Staging st\(ctx, "(prs_\w+)"', open(os.path.join(csrc, f)).read()))
    assert named == set(STAGING) - {"prs_pose_graph_optimize", "prs_pose_graph_optimize_lm"}  # (those two pass their name in: `entry`)


# ---- 4. handles ------------------------------------------------------------------------------------------------------------------
def test_projective_finder_with_the_fixed_cloud_at_the_handles_capacity(oracle, monkeypatch):
    """a first cloud of 300 points sizes the block for 512 (pcf_api.hip, ensure_capacity); the second one fills it to the last row"""
    cfg, fixed, dfix, mp, T, X0 = make_align_case("kitti", 12, 900, 900)
    assert len(fixed) >= 512
    fixed, dfix = fixed[:512], dfix[:512]
    scale = oracle.info_scale_from_nopt(mp["n_opt"])
    of_ = oracle.ProjectiveFinder(finder.pcf_params_from_cfg(oracle, cfg))
    of_.set_fixed(fixed, dfix)
    of_.set_moving(mp["xyz"], mp["desc"])
    of_.set_local_map_in_sensor(X0)
    rc0, rflags0 = of_.compute()
    md = oracle.mean_disparity(fixed)
    res, rcorr = oracle.align_frame(of_, finder.oracle_aligner_params(oracle, cfg, mean_disparity=md), fixed, mp["xyz"], scale, X0)
    assert len(rc0) > 100 and len(rcorr) > 100

    def run(ctx, fill):
        gf = ops.ProjectiveFinder(ctx, ops.pcf_params(cfg))
        gf.set_fixed(fixed[:300], dfix[:300])
        gf.set_moving(mp["xyz"], mp["desc"], scale)
        block = [r for r in ctx.guard_regions() if r["name"] == "pcf.d_block"]
        gf.set_fixed(fixed, dfix)
        assert [r for r in ctx.guard_regions() if r["name"] == "pcf.d_block"] == block, "512 points fit the block made for 300"
        gf.set_local_map_in_sensor(X0)
        gc, gflags = gf.compute()
        assert corr_equal(rc0, gc) and gflags == rflags0
        Xg, gcorr, gres, gflags = gf.align(ops.aligner_params(cfg, stop_at_fixed_point=1), X0)
        assert corr_equal(rcorr, gcorr) and np.array_equal(finder._bits(np.array(res.X)), finder._bits(Xg.reshape(-1)))
        assert (res.status, res.num_inliers, res.num_correspondences, res.warnings) == (gres.status, gres.num_inliers, gres.num_correspondences, gflags)
        assert finder._same_state(of_, gf)
        note(ctx, "ProjectiveFinder with its handle, fill %02x" % fill)
        assert ctx.guard_check() == 0
        gf.close()  # its two blocks are checked as they go
        assert not {"pcf.d_block", "pcf.h_block"} & set(names_of(ctx))
        return dict(compute=gc, corr=gcorr, X=Xg)

    under_both_fills(monkeypatch, "ProjectiveFinder", run, JOB[:4])


MAP_ARRAYS = ["map." + k for k in ("coords", "desc", "state", "cov", "n_opt", "inlier", "n_meas", "meas", "poses", "measurement", "mdesc", "corr",
                                   "index_map", "small")]


def test_map_handle_merged_until_it_is_full_then_a_closure_merge(monkeypatch):
    """three frames of tests/merge_cases.py through prs_map_merge, every readable array against the checker, in a map whose capacity
    is exactly what they fill; then the closure merger's `exactly_full` measurement on that map, against the default path; then
    that case on a handle of its own, against tests/closure_merge_ref.py, as the closure merger's own test runs it"""
    kind, frames = "stereo_ekf", 3
    seq = mc.Sequence(kind, 2100, 200, frames, response_max=50)
    P = mc.merger_params(kind, 1)
    dry, poses = seq.new_map(4096), om.pose_table(frames)
    for k in range(frames):
        Tw, Ts, z, desc, corr = seq.inputs(k, dry)
        assert om.merge(P, Tw, Ts, poses, k, dry, z, desc, corr)[0] == 0
    cap = dry.n_points
    assert cap > 150
    c = cc.edge("exactly_full")
    plain = dict(c, scene=closure_sizes.plain_scene(c), scene_in_world=np.eye(4, dtype=F))
    S, r, _ = cc.want(plain)
    assert S["n_points"] == len(S["coords"]) and r[1] > 0, "the closure case fills its scene to the last row"
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)  # noqa: E731

    def merged_to_capacity(ctx):
        m, table = seq.new_map(cap), om.pose_table(frames)
        h = ops.MapHandle(ctx, cap, seq.max_meas, max_frames=frames, max_measured=1024)
        for k in range(frames):
            Tw, Ts, z, desc, corr = seq.inputs(k, m)
            rc, res = om.merge(P, Tw, Ts, table, k, m, z, desc, corr)
            assert rc == 0 and h.merge(merge.gpu_params(P), Tw, Ts, z, desc, corr) == (res.n_merged, res.n_added, res.flags), k
            sc, n = h.scene(), m.n_points
            assert h.size() == (n, k + 1)
            assert np.array_equal(bits(sc["coords"]), bits(m.coords[:n, :3])) and np.array_equal(bits(sc["state"]), bits(m.state[:n, :3])), k
            assert np.array_equal(sc["desc"], m.desc[:n]) and np.array_equal(sc["n_opt"], m.n_opt[:n]) and np.array_equal(sc["inlier"], m.inlier[:n]), k
        assert h.size()[0] == cap == h.capacity, "n_points == capacity"
        res = h.merge_closure(closure.params_of(c["P"]), c["transform"], c["measurement"], c["measurement_desc"], c["corr"], check=False)
        return h, dict(res=np.array(res, np.int32), **h.scene())

    plain_ctx = ops.Context(0)
    try:
        h0, want = merged_to_capacity(plain_ctx)
        h0.close()
    finally:
        plain_ctx.close()

    def run(ctx, fill):
        h, got = merged_to_capacity(ctx)
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), ("closure merge into the full map", k)
        note(ctx, "MapHandle with its handle, fill %02x" % fill)
        assert ctx.guard_check() == 0 and set(MAP_ARRAYS) <= set(names_of(ctx))
        h.close()
        n = plain["scene"]["n_points"]
        m = ops.MapHandle(ctx, len(plain["scene"]["coords"]), max_measured=512)
        m.set_scene(plain["scene"]["coords"][:n, :3], plain["scene"]["desc"][:n])
        assert m.merge_closure(closure.params_of(c["P"]), c["transform"], c["measurement"], c["measurement_desc"], c["corr"]) == r
        closure_sizes.handle_scene_equals(m, S)
        assert m.size()[0] == m.capacity
        assert ctx.guard_check() == 0
        full = m.scene()
        m.close()
        return as_arrays(dict(first=got, second=full))

    under_both_fills(monkeypatch, "MapHandle", run)


DB_ARRAYS = ["place_db." + k for k in ("desc", "xyz", "row_pidx", "tile_map", "map_off", "map_rows", "map_gid")]
BANK_ARRAYS = ["place_bank." + k for k in ("desc", "xyz", "row_pidx", "tile_map", "map_off", "map_rows", "map_gid", "own_nodes", "counters")]


def test_place_database_across_a_growth_of_rows_and_of_maps(monkeypatch):
    """18 maps of 64 rows: the 17th does not fit the 16 maps the first one reserved, the 18th not its 1088 rows, so every array is
    copied into a larger block (grow copies old_n elements: what the check sees); then queries through both entries against
    tests/place_ref.py"""
    rng = np.random.default_rng(77)
    base = plc.random_rows(rng, 64)
    maps = [bank.near(rng, base, 64) for _ in range(18)]
    xyz = rng.integers(-50, 50, (64, 3)).astype(F)
    P = bank.params(ops, max_candidates=24)  # (room for every stored map: more candidates than that is PRS_ERR_CAPACITY)

    def run(ctx, fill):
        pair = plc.Pair(ctx, ops)
        sizes = []
        for g, d in enumerate(maps):
            pair.add(g, d, xyz)
            sizes.append({r["name"]: r["bytes"] for r in ctx.guard_regions() if r["name"] in DB_ARRAYS})
        assert pair.dev.size()[:2] == (18, 18 * 64) and sorted(sizes[0]) == sorted(DB_ARRAYS)
        assert all(sizes[-1][k] > sizes[0][k] for k in DB_ARRAYS), "every array has grown, with maps stored in it"
        out = []
        for g in (18, 19):
            q = bank.near(np.random.default_rng(g), base, 80)
            want = plc.both_entries(ctx, ops, pair, P, g, q, what="query %d" % g)
            assert want["candidates"], "the query finds stored maps"
            out.append(pair.dev.query(P, g, q))
        note(ctx, "PlaceDatabase with its handle, fill %02x" % fill)
        assert ctx.guard_check() == 0 and set(DB_ARRAYS) <= set(names_of(ctx))
        pair.dev.close()
        return as_arrays(out)

    under_both_fills(monkeypatch, "PlaceDatabase", run, ["arena.pinned", "arena.stage"])


def test_place_bank_filled_to_its_last_row(monkeypatch):
    """the bank test's growth walk: sequence 1 ends with 1088 rows in a row_stride of 1088 and refuses the next map, the twin
    databases grow with the host add(); both references of that test, on guarded blocks"""
    base = plc.random_rows(np.random.default_rng(2024), 64)

    def run(ctx, fill):
        seen, real = [], bank.Rig.check_query
        with monkeypatch.context() as m:
            m.setattr(bank.Rig, "check_query", lambda self, items, got, what="": seen.append(got) or real(self, items, got, what))
            m.setattr(bank.Rig, "close", lambda self: (seen.append(names_of(ctx)), note(ctx, "PlaceBank with its handles, fill %02x" % fill),
                                                       self.bank.close(), [t.close() for t in self.twins or []]))
            bank.test_growth_against_both_references((ctx, ops), base)
        assert set(BANK_ARRAYS + DB_ARRAYS) <= set(seen[-1])
        return as_arrays(seen[:-1])

    under_both_fills(monkeypatch, "PlaceBank", run)


# ---- 5. the harness itself -------------------------------------------------------------------------------------------------------
class _Raw:
    """`n` bytes of device memory at `ptr` for torch.as_tensor"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(int(n),), typestr="|u1", data=(int(ptr), False), version=2)


def poke(ptr, value):
    """one byte of device memory; the address lies inside an allocation of the library, bands included"""
    try:
        torch.as_tensor(_Raw(ptr, 1), device="cuda").fill_(value)
        torch.cuda.synchronize()
    except (TypeError, RuntimeError, ValueError):
        # this torch build takes no foreign pointer: one byte through the HIP runtime the process has loaded
        path = [line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line][0]
        hip = C.CDLL(path)
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        byte = C.c_uint8(value)
        assert hip.hipMemcpy(C.c_void_p(ptr), C.byref(byte), 1, 1) == 0  # (hipMemcpyHostToDevice)


def region(ctx, name):
    r, = [r for r in ctx.guard_regions() if r["name"] == name]
    return r


@pytest.mark.parametrize("where", ["first", "last"])
def test_one_damaged_byte_of_a_tail_band_is_reported_by_name_side_and_offset(monkeypatch, where):
    call = staging._triangulate(64)
    ctx = guarded_context(monkeypatch, 0xFF)
    try:
        call(ctx)
        assert ctx.guard_check() == 0
        r = region(ctx, "arena.stage")
        assert not r["pinned"] and r["tail_bytes"] >= guarded.MIN_BAND and r["user"] % 256 == 0
        offset = 0 if where == "first" else r["tail_bytes"] - 1
        poke(r["user"] + r["bytes"] + offset, 0x3C)
        assert ctx.guard_check(report=True) == (1, ["arena.stage tail %d" % offset])
        assert ctx.guard_check(report=True) == (1, ["arena.stage tail %d" % offset]), "a check changes nothing"
        call(ctx)  # the block is reused and painted again: the bands are not
        assert ctx.guard_check() == 1
    finally:
        ctx.close()
    assert ctx.close_status == 1


def test_the_front_band_and_the_pinned_mirror_are_checked_too(monkeypatch):
    call = staging._triangulate(64)
    ctx = guarded_context(monkeypatch, 0x00)
    try:
        call(ctx)
        r, p = region(ctx, "arena.stage"), region(ctx, "arena.pinned")
        poke(r["user"] - 1, 0x3C)
        assert p["pinned"]
        C.memset(p["user"] + p["bytes"] + 7, 0x3C, 1)  # (pinned host memory: the band is checked on the host)
        assert ctx.guard_check(report=True) == (2, ["arena.stage front %d" % (guarded.MIN_BAND - 1), "arena.pinned tail 7"])
    finally:
        ctx.close()
    assert ctx.close_status == 2


def test_a_violation_stays_latched_when_growth_frees_the_damaged_block(monkeypatch):
    small, large = staging._triangulate(64), staging._triangulate(60000)
    ctx = guarded_context(monkeypatch, 0xFF)
    try:
        small(ctx)
        r = region(ctx, "arena.stage")
        poke(r["user"] + r["bytes"] + 5, 0x3C)
        large(ctx)  # the arena grows: the damaged block is checked, latched and freed
        grown = region(ctx, "arena.stage")
        assert grown["bytes"] > r["bytes"]
        assert ctx.guard_check(report=True) == (1, ["arena.stage tail 5"]), "the evidence outlives its block"
        small(ctx)
        assert ctx.guard_check(report=True) == (1, ["arena.stage tail 5"])
    finally:
        ctx.close()
    assert ctx.close_status == 1, "nor does prs_context_destroy lose it"
