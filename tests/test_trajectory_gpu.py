"""The trajectory evaluator on the device (csrc/trajectory.hip, prs_trajectory_eval_batch) against the float64 numpy restatement of its
definitions (tests/trajectory_ref.py): every field of the result, frame_error and the cumulative distances, at the shapes where the
kernel changes path (fewer rows than the alignment needs, one wave, one workgroup pass, several; staged and unstaged clouds), under
every alignment and mask, with the KITTI block's subsequence selection compared exactly.

Tolerance (derived, not measured): both sides form float64 sums of at most 4541 terms of the same float32 inputs, in different orders:
K * 2^-53 = 5e-13 relative.  The bound is |got - want| <= 1e-9 * (|want| + scale) with scale = 1 for angles, ratios and rotation
entries and the largest |coordinate| of the two clouds for lengths, which leaves three orders of magnitude for the eigen-solver's
iteration.  frame_error is float32: one rounding (2^-24 relative) is added."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import trajectory_ref as tr
from srrg2_proslam_amd import _lib, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-9
LENGTH_FIELDS = ("path_length", "ate_rmse", "ate_mean", "ate_max", "rpe_t_rmse", "rpe_t_mean", "rpe_t_max", "axis_t_mean", "axis_t_std")
UNIT_FIELDS = ("rpe_r_rmse", "rpe_r_mean", "rpe_r_max", "axis_r_mean", "axis_r_std", "kitti_t", "kitti_r", "kitti_t_len", "kitti_r_len")
COUNT_FIELDS = ("status", "n_valid", "n_rpe", "n_kitti", "kitti_n_len")
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def ctx():
    c = ops.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gt():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_kitti_gt.npz"))
    return {"city": tr.to44(z["city"]), "highway": tr.to44(z["highway"])}


def _rot(rv):
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def drifted(G, seed):
    """the ground truth composed with seeded drift: per-frame rotation noise <= 0.01 rad and translation noise <= 0.05 m, accumulated;
    float32 [n, 16]"""
    rng = np.random.default_rng(seed)
    n = G.shape[0]
    out = np.empty((n, 4, 4))
    D = np.eye(4)
    for k in range(n):
        d = np.eye(4)
        axis = rng.normal(size=3)
        d[:3, :3] = _rot(axis / np.linalg.norm(axis) * rng.uniform(0, 0.01))
        step = rng.normal(size=3)
        d[:3, 3] = step / np.linalg.norm(step) * rng.uniform(0, 0.05)
        D = D @ d
        out[k] = G[k] @ D
    return out.reshape(n, 16).astype(np.float32)


def rows16(G):
    return G.reshape(-1, 16).astype(np.float32)


def padded(rows, stride):
    """rows [n, 16] -> [stride, 16] with NaN from n on: a row past n_frames must never reach a sum"""
    out = np.full((stride, 16), np.nan, np.float32)
    out[:rows.shape[0]] = rows
    return out


class Batch:
    """sequences of (estimate [stride, 16], ground truth [stride, 16], n_frames, valid or None) on the device, outputs pre-filled"""

    def __init__(self, seqs, stride, with_valid):
        self.seqs, self.stride = seqs, stride
        self.ev = ev = ops.TrajectoryEvalBatch(0, len(seqs), stride, with_valid=with_valid)
        est = np.stack([s[0] for s in seqs])
        g = np.stack([s[1] for s in seqs])
        ev.estimate.copy_(torch.from_numpy(est).reshape(len(seqs), stride, 16))
        ev.ground_truth.copy_(torch.from_numpy(g).reshape(len(seqs), stride, 16))
        ev.n_frames.copy_(torch.tensor([s[2] for s in seqs], dtype=torch.int32))
        if with_valid:
            ev.valid.copy_(torch.from_numpy(np.stack([np.ones(stride, np.uint8) if s[3] is None else s[3] for s in seqs])))
        ev.workspace.fill_(SENTINEL)
        ev.frame_error.fill_(SENTINEL)

    def run(self, ctx, params):
        self.ev.evaluate(ctx, params)
        torch.cuda.synchronize()
        return self.ev.results(), self.ev.frame_error.cpu().numpy(), self.ev.workspace.cpu().numpy()


def ref_of(seq, align=tr.ALIGN_RIGID, rpe_delta=1, kitti_step=10, lengths=tr.KITTI_LENGTHS):
    return tr.evaluate(seq[0], seq[1], n_frames=seq[2], valid=seq[3], align=align, rpe_delta=rpe_delta, kitti_step=kitti_step, lengths=lengths)


def cloud_scale(seq):
    n = min(max(seq[2], 0), seq[0].shape[0])
    ok = np.ones(n, bool) if seq[3] is None else seq[3][:n] != 0
    t = np.concatenate([seq[0][:n][ok][:, [3, 7, 11]], seq[1][:n][ok][:, [3, 7, 11]]]).astype(np.float64)
    return float(np.abs(t).max()) if t.size else 0.0


def check(got, ferr, want, scale, what):
    """every field of one result and its frame_error row against the restatement"""
    for k in COUNT_FIELDS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k, got[k], want[k])
    for fields, s in ((LENGTH_FIELDS, scale), (UNIT_FIELDS, 1.0)):
        for k in fields:
            g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
            err = np.abs(g - w)
            print("%s %s: got %s want %s err %s" % (what, k, g, w, err))
            assert np.all(err <= REL * (np.abs(w) + s)), (what, k, g, w)
    g, w = got["S"], want["S"]
    assert np.all(np.abs(g[:3, :3] - w[:3, :3]) <= REL * (np.abs(w[:3, :3]) + 1.0)), (what, "S rotation", g, w)
    assert np.all(np.abs(g[:3, 3] - w[:3, 3]) <= REL * (np.abs(w[:3, 3]) + scale)), (what, "S translation", g, w)
    assert np.array_equal(g[3], [0, 0, 0, 1])
    w = want["frame_error"]
    assert ferr.shape == w.shape
    assert np.array_equal(ferr == -1, w == -1), (what, "frame_error mask")
    assert np.all(np.abs(ferr - w) <= REL * (np.abs(w) + scale) + 2.0 ** -24 * np.abs(w)), (what, "frame_error", np.abs(ferr - w).max())


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
SHAPES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1101, 4541)
SHAPE_STRIDE = 4544


@pytest.fixture(scope="module")
def shapes(ctx, gt):
    """one launch over the twelve lengths, rigid alignment, delta 1, the devkit's KITTI block"""
    est = {"highway": drifted(gt["highway"], 11), "city": drifted(gt["city"], 12)}
    seqs = []
    for n in SHAPES:
        src = "city" if n > 1101 else "highway"
        seqs.append((padded(est[src][:n], SHAPE_STRIDE), padded(rows16(gt[src][:n]), SHAPE_STRIDE), n, None))
    b = Batch(seqs, SHAPE_STRIDE, with_valid=False)
    return b, b.run(ctx, ops.trajectory_params())


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["n%d" % n for n in SHAPES])
def test_shapes(shapes, i):
    b, (res, ferr, work) = shapes
    seq, n = b.seqs[i], SHAPES[i]
    want = ref_of(seq)
    if n < 3:
        assert want["status"] == tr.ERR_RANGE and res[i]["status"] == tr.ERR_RANGE
        assert res[i]["n_valid"] == n and res[i]["ate_rmse"] == 0.0 and np.array_equal(res[i]["S"], np.eye(4))
    else:
        assert want["status"] == 0 and want["kitti_margin"] >= 1e-6
    check(res[i], ferr[i], want, cloud_scale(seq), "n=%d" % n)
    # the cumulative distances, and nothing written past the sequence's rows
    if n >= 3:
        dist = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(seq[1][:n, [3, 7, 11]].astype(np.float64), axis=0), axis=1))])
        assert np.all(np.abs(work[i, :n] - dist) <= REL * (dist + cloud_scale(seq)))
        assert abs(res[i]["path_length"] - dist[-1]) <= REL * (dist[-1] + cloud_scale(seq))
    assert np.all(work[i, n if n >= 3 else 0:] == SENTINEL)


@pytest.mark.parametrize("stride", [4800, 4801, 6400, 6401])
def test_stage_limits_give_the_same_bytes(ctx, gt, shapes, stride):
    """frame_stride at and past the two LDS limits: up to 4800 rows the clouds and the cumulative distances are staged, up to 6400 the
    clouds alone, beyond nothing; the passes then read global memory with the same arithmetic"""
    b, _ = shapes
    picks = [SHAPES.index(65), SHAPES.index(257), SHAPES.index(1101)]
    seqs = [(padded(b.seqs[i][0][:SHAPES[i]], stride), padded(b.seqs[i][1][:SHAPES[i]], stride), SHAPES[i], None) for i in picks]
    got = Batch(seqs, stride, with_valid=False)
    res, ferr, work = got.run(ctx, ops.trajectory_params())
    staged = b.ev.result.cpu().numpy()
    for j, i in enumerate(picks):
        check(res[j], ferr[j], ref_of(seqs[j]), cloud_scale(seqs[j]), "stride %d n=%d" % (stride, SHAPES[i]))
        assert np.array_equal(got.ev.result.cpu().numpy()[j], staged[i])
        assert np.array_equal(work[j, :SHAPES[i]], shapes[1][2][i, :SHAPES[i]]) and np.all(work[j, SHAPES[i]:] == SENTINEL)


# ---- alignment ---------------------------------------------------------------------------------------------------------------------
def test_alignment(ctx, gt):
    G = gt["highway"][:257]
    n, stride = 257, 260
    est = drifted(G, 21).reshape(n, 4, 4).astype(np.float64)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _rot(np.array([0.3, -1.0, 0.2]) / np.linalg.norm([0.3, -1.0, 0.2]) * 2.5), [1000.0, -20.0, 300.0]
    far = rows16(T @ est)
    # planar ground truth (y = 0) and its mirror image (x -> -x), exactly planar and 0.5 m out of the plane
    flat = rows16(G).copy()
    flat[:, 7] = 0.0
    mirror = flat.copy()
    mirror[:, 3] = -mirror[:, 3]
    bumpy = flat.copy()
    bumpy[:, 7] = np.random.default_rng(22).uniform(-0.5, 0.5, n).astype(np.float32)
    bumpy_mirror = bumpy.copy()
    bumpy_mirror[:, 3] = -bumpy_mirror[:, 3]
    g16 = rows16(G)
    seqs = [(padded(far, stride), padded(g16, stride), n, None), (padded(mirror, stride), padded(flat, stride), n, None),
            (padded(bumpy_mirror, stride), padded(bumpy, stride), n, None), (padded(rows16(est), stride), padded(g16, stride), n, None)]
    b = Batch(seqs, stride, with_valid=False)
    for name, align in (("rigid", tr.ALIGN_RIGID), ("first", tr.ALIGN_FIRST), ("none", tr.ALIGN_NONE)):
        res, ferr, _ = b.run(ctx, ops.trajectory_params(align=name, kitti_step=0))
        for i, seq in enumerate(seqs):
            check(res[i], ferr[i], ref_of(seq, align=align, kitti_step=0), cloud_scale(seq), "%s seq %d" % (name, i))
            if align == tr.ALIGN_RIGID:
                R = res[i]["S"][:3, :3]
                assert abs(np.linalg.det(R) - 1.0) <= 1e-12 and np.all(np.abs(R @ R.T - np.eye(3)) <= 1e-12)
        if align == tr.ALIGN_RIGID:
            # centring: the kilometre and the 2.5 rad are taken out, what is left is the drift's own residual
            assert abs(res[0]["ate_rmse"] - res[3]["ate_rmse"]) < 1e-2
            assert np.all(np.abs(res[0]["S"] @ T - res[3]["S"]) < 1e-2)
            assert res[1]["ate_max"] < 1e-9  # the exactly planar mirror image is a half turn away
            assert res[2]["ate_rmse"] > 0.1  # the bumpy one is not: a reflection would reach 0, a rotation cannot


# ---- masks -------------------------------------------------------------------------------------------------------------------------
def test_masks(ctx, gt):
    n, stride = 257, 259
    G = rows16(gt["highway"][:n])
    P = drifted(gt["highway"][:n], 31)
    masks = {"all": np.ones(stride, np.uint8), "first": np.ones(stride, np.uint8), "last": np.ones(stride, np.uint8),
             "alternate": np.ones(stride, np.uint8), "none": np.zeros(stride, np.uint8)}
    masks["first"][0] = 0
    masks["last"][n - 1] = 0
    masks["alternate"][1::2] = 0
    seqs = []
    for name, m in masks.items():
        p, g = padded(P, stride), padded(G, stride)
        p[m == 0] = np.nan  # an invalid row must not reach a sum either
        g[m == 0] = np.nan
        seqs.append((p, g, n, m))
    b = Batch(seqs, stride, with_valid=True)
    for delta in (1, 10, n - 1, n):
        res, ferr, _ = b.run(ctx, ops.trajectory_params(rpe_delta=delta, kitti_step=3, lengths=(5, 10, 20, 40, 80, 160)))
        for i, name in enumerate(masks):
            want = ref_of(seqs[i], rpe_delta=delta, kitti_step=3, lengths=(5, 10, 20, 40, 80, 160))
            check(res[i], ferr[i], want, cloud_scale(seqs[i]), "mask %s delta %d" % (name, delta))
            assert (res[i]["n_kitti"] > 0) == (name == "all")
            if name == "none":
                assert res[i]["status"] == tr.ERR_RANGE and res[i]["n_valid"] == 0
            if delta == n:
                assert res[i]["n_rpe"] == 0 and res[i]["rpe_t_rmse"] == 0.0
        assert res[0]["n_rpe"] == n - delta and res[3]["n_rpe"] == (0 if delta % 2 else max((n - delta + 1) // 2, 0))


# ---- the KITTI block ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, step, lengths, count", [(4541, 10, tr.KITTI_LENGTHS, 3283), (400, 5, (10, 20, 40, 80), 279),
                                                        (257, 3, (5, 10, 20, 40, 80, 160), 361)])
def test_kitti_block(ctx, gt, rows, step, lengths, count):
    G = gt["city"][:rows]
    stride = rows + 1
    seq = (padded(drifted(G, 41), stride), padded(rows16(G), stride), rows, None)
    want = ref_of(seq, kitti_step=step, lengths=lengths)
    # no summation order can move an index: every selected dist[last] and dist[last - 1] is at least 1e-6 m from its threshold
    assert want["kitti_margin"] >= 1e-6 and want["n_kitti"] == count
    res, ferr, _ = Batch([seq], stride, with_valid=False).run(ctx, ops.trajectory_params(kitti_step=step, lengths=lengths))
    assert res[0]["n_kitti"] == want["n_kitti"] and np.array_equal(res[0]["kitti_n_len"], want["kitti_n_len"])
    check(res[0], ferr[0], want, cloud_scale(seq), "kitti %d rows" % rows)


# ---- independence and determinism ----------------------------------------------------------------------------------------------------
def test_independence_and_determinism(ctx, gt, shapes):
    b, _ = shapes
    picks = [SHAPES.index(n) for n in (3, 64, 65, 257, 1101, 255, 4541)]
    seqs = [b.seqs[i] for i in picks]
    together = Batch(seqs, SHAPE_STRIDE, with_valid=False)
    together.run(ctx, ops.trajectory_params())
    first = together.ev.result.cpu().numpy().copy()
    first_err = together.ev.frame_error.cpu().numpy().copy()
    together.ev.result.zero_()
    together.run(ctx, ops.trajectory_params())
    assert np.array_equal(together.ev.result.cpu().numpy(), first) and np.array_equal(together.ev.frame_error.cpu().numpy(), first_err)
    for j, seq in enumerate(seqs):
        alone = Batch([seq], SHAPE_STRIDE, with_valid=False)
        alone.run(ctx, ops.trajectory_params())
        assert np.array_equal(alone.ev.result.cpu().numpy()[0], first[j]), "sequence %d depends on its batch" % j
        assert np.array_equal(alone.ev.frame_error.cpu().numpy()[0], first_err[j])
    # nor on the stride it is stored at
    n = 257
    tight = Batch([(seqs[3][0][:n + 1], seqs[3][1][:n + 1], n, None)], n + 1, with_valid=False)
    tight.run(ctx, ops.trajectory_params())
    assert np.array_equal(tight.ev.result.cpu().numpy()[0], first[3])


# ---- in place and captured -----------------------------------------------------------------------------------------------------------
def test_in_place_on_a_session_and_captured(ctx, gt):
    B, stride, ns = 2, 70, (65, 40)
    maps, frames = ops.MapBatch(0, B, 16, 1, 4, 1, 1), ops.AlignFrames(0, B, 1, 1)
    graphs = ops.PoseGraphBatch(0, B, 8, 8, envelope_blocks=32)
    sess = ops.SessionBatch(0, maps, frames, graphs, stride)
    G = rows16(gt["highway"][:stride])
    ests = [drifted(gt["highway"][:stride], 51), drifted(gt["highway"][:stride], 52)]
    # a hand-filled log in node 0 (X = I): the unroll writes these rows into sess.trajectory
    sess.frame_pose.copy_(torch.from_numpy(np.stack(ests)).reshape(B, stride, 16))
    sess.n_frames.copy_(torch.tensor(ns, dtype=torch.int32))
    ev = ops.TrajectoryEvalBatch.from_session(sess, with_valid=False)
    assert ev.estimate.data_ptr() == sess.trajectory.data_ptr() and ev.n_frames.data_ptr() == sess.n_frames.data_ptr()
    d = ev.descriptor()
    assert d.estimate == sess.trajectory.data_ptr() and d.n_frames == sess.n_frames.data_ptr()
    for b_ in range(B):
        ev.set_ground_truth(b_, G)
    params = ops.trajectory_params(kitti_step=5, lengths=(10, 20, 40))
    ctx.use_torch_stream()
    sess.unroll(ctx)
    ev.evaluate(ctx, params)
    torch.cuda.synchronize()
    eager = ev.result.cpu().numpy().copy()
    res = ev.results()
    ferr = ev.frame_error.cpu().numpy()
    for b_ in range(B):
        seq = (ests[b_], G, ns[b_], None)
        check(res[b_], ferr[b_], ref_of(seq, kitti_step=5, lengths=(10, 20, 40)), cloud_scale(seq), "session %d" % b_)
    # one captured launch: a linear graph that replays to the eager bytes, also after the trajectory changed and changed back
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        ev.evaluate(ctx, params)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ev.evaluate(ctx, params)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    ev.result.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(ev.result.cpu().numpy(), eager)
    sess.n_frames.copy_(torch.tensor((40, 65), dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    swapped = ev.results()
    assert swapped[0]["n_valid"] == 40 and swapped[1]["n_valid"] == 65
    check(swapped[0], ev.frame_error.cpu().numpy()[0], ref_of((ests[0], G, 40, None), kitti_step=5, lengths=(10, 20, 40)),
          cloud_scale((ests[0], G, 40, None)), "replayed")


def test_host_array_convenience(ctx, gt):
    G = gt["highway"][:65]
    P = drifted(G, 61)
    valid = np.ones(65, np.uint8)
    valid[7] = 0
    got = ops.trajectory_eval(ctx, ops.trajectory_params(kitti_step=0), P, G, valid=valid)
    seq = (P, rows16(G), 65, valid)
    check(got, got["frame_error"], ref_of(seq, kitti_step=0), cloud_scale(seq), "host arrays")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
NULL, RANGE, UNSUPPORTED = -1, -4, -5


def test_refusals_leave_the_outputs_untouched(ctx, gt):
    n, stride = 65, 66
    G = rows16(gt["highway"][:n])
    seq = (padded(drifted(gt["highway"][:n], 71), stride), padded(G, stride), n, None)
    b = Batch([seq, seq], stride, with_valid=True)
    b.ev.result.fill_(0xAB)
    lib = _lib.load()

    def call(params=None, **fields):
        p = params if params is not None else ops.trajectory_params()
        d = b.ev.descriptor()
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.prs_trajectory_eval_batch(ctx._h, C.byref(p), C.byref(d))

    def with_lengths(*v):
        return ops.trajectory_params(lengths=v)

    def field(**kv):
        p = ops.trajectory_params()
        for k, v in kv.items():
            setattr(p, k, v)
        return p

    d0 = b.ev.descriptor()
    cases = [
        (NULL, call(estimate=None)), (NULL, call(ground_truth=None)), (NULL, call(n_frames=None)), (NULL, call(result=None)),
        (NULL, call(workspace=None)),  # kitti_step > 0
        (NULL, lib.prs_trajectory_eval_batch(ctx._h, None, C.byref(d0))),
        (NULL, lib.prs_trajectory_eval_batch(ctx._h, C.byref(ops.trajectory_params()), None)),
        (RANGE, call(batch=0)), (RANGE, call(frame_stride=0)), (RANGE, call(batch=-1)),
        (RANGE, call(field(rpe_delta=0))), (RANGE, call(field(kitti_step=-1))), (RANGE, call(field(n_lengths=9))),
        (RANGE, call(field(n_lengths=-1))), (RANGE, call(field(align=3))), (RANGE, call(field(align=-1))),
        (RANGE, call(with_lengths(10, float("nan")))), (RANGE, call(with_lengths(10, float("inf")))), (RANGE, call(with_lengths(0.0, 10))),
        (RANGE, call(with_lengths(-5.0, 10))), (RANGE, call(with_lengths(10, 20, 20))), (RANGE, call(with_lengths(10, 30, 20))),
        (UNSUPPORTED, call(estimate=d0.estimate + 4)), (UNSUPPORTED, call(ground_truth=d0.ground_truth + 8)),
        (UNSUPPORTED, call(result=d0.result + 4)), (UNSUPPORTED, call(workspace=d0.workspace + 4)),
    ]
    for i, (want, got) in enumerate(cases):
        assert got == want, (i, want, got)
    torch.cuda.synchronize()
    assert bool((b.ev.result == 0xAB).all()) and bool((b.ev.frame_error == SENTINEL).all()) and bool((b.ev.workspace == SENTINEL).all())
    # not refusals: no workspace without the KITTI block, no frame_error, no lengths; and a negative n_frames is its sequence's alone
    b.ev.n_frames[1] = -1
    assert call(field(kitti_step=0), workspace=None, frame_error=None, valid=None) == 0
    assert call(with_lengths()) == 0
    torch.cuda.synchronize()
    res = b.ev.results()
    assert res[1]["status"] == RANGE and res[1]["n_valid"] == 0 and res[1]["ate_rmse"] == 0.0
    check(res[0], b.ev.frame_error.cpu().numpy()[0], ref_of(seq, lengths=()), cloud_scale(seq), "beside a refused sequence")
    assert bool((b.ev.frame_error[1] == -1).all())
