"""The pose algebra of csrc/prs_se3.h on the device, reached directly through the C-ABI: prs_motion_predict_batch,
prs_pose_compose_batch, prs_gn_step / prs_gn_step_ex and the pose-graph optimisers, on the cases of tests/pose_algebra_cases.py --
rotations beyond 120 degrees in every largest-diagonal branch of t2tnq, the q0 < 0 sign flip, tied diagonals, half turns, rotation
blocks off SO(3), large translations; pivots that are negative, zero, NaN, denormal, 2^127 and infinite; steps of |dq| >= 1 --
against the CPU oracle bit for bit (tests/test_pose_algebra_ref.py holds the oracle to float64)."""
import ctypes as C

import numpy as np
import pytest
import torch

import pose_algebra_cases as pa
import pose_graph_lm_ref as lm
import pose_graph_ref as pg
from srrg2_proslam_amd import _lib, configs, ops
from test_pose_graph_gpu import assert_same as assert_same_gn
from test_pose_graph_lm_gpu import assert_same as assert_same_lm

pytestmark = pytest.mark.gpu
f32 = np.float32
BATCHES = (1, 255, 256, 257, 513)  # the kernels' blocks are 256 threads
PLANT = -12345.5


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.fixture
def variant(oracle):
    yield oracle.set_variant
    oracle.set_variant()


_rows = {}


def predict_rows(oracle):
    """(P2 [N, 4, 4], P1, the oracle's prediction): every pose case as P1, with each kind of P2; built once"""
    if "predict" not in _rows:
        P1 = np.stack([c["T"] for c in pa.poses() for _ in pa.P2_KINDS])
        P2 = np.stack([pa.previous_pose(c["T"], kind) for c in pa.poses() for kind in pa.P2_KINDS])
        want = np.stack([oracle.motion_predict(a, b) for a, b in zip(P2, P1)])
        _rows["predict"] = (P2, P1, want)
    return _rows["predict"]


def compose_rows(oracle):
    """(prediction, X, the oracle's prediction * X^-1): every pose case in both places (X = the case 7 further on)"""
    if "compose" not in _rows:
        Ts = np.stack([c["T"] for c in pa.poses()])
        Xs = np.roll(Ts, -7, axis=0)
        want = np.stack([oracle.se3_mul(p, oracle.se3_inverse(x)) for p, x in zip(Ts, Xs)])
        _rows["compose"] = (Ts, Xs, want)
    return _rows["compose"]


def _run(hip_ctx, op, a, b, batch, rows_out):
    hip_ctx.use_torch_stream()
    da, db = torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
    out = torch.full((rows_out, 4, 4), PLANT, dtype=torch.float32, device=da.device)
    assert batch <= len(a) and batch <= rows_out
    op(hip_ctx, da[:batch].contiguous(), db[:batch].contiguous(), out)  # (the operators take the batch size from their inputs)
    hip_ctx.synchronize()
    return out.cpu().numpy()


def _spread(n_rows, batch):
    """`batch` row indices spread over all the cases (so that every batch size holds every branch), the first repeated at the end"""
    idx = np.linspace(0, n_rows - 1, batch).astype(np.int64)
    if batch > 1:
        idx[-1] = idx[0]
    return idx


def test_motion_predict_every_case(oracle, hip_ctx):
    P2, P1, want = predict_rows(oracle)
    got = _run(hip_ctx, ops.motion_predict_batch, P2, P1, len(P1), len(P1) + 3)
    bad = [i for i in range(len(P1)) if not np.array_equal(_bits(got[i]), _bits(want[i]))]
    names = [(pa.poses()[i // len(pa.P2_KINDS)]["name"], pa.P2_KINDS[i % len(pa.P2_KINDS)]) for i in bad[:5]]
    assert not bad, (len(bad), names)
    assert np.all(got[len(P1):] == PLANT)
    # the batch reaches every branch of t2tnq on the raw prediction, both signs of q0, and the carried-w path
    raw = [oracle.se3_mul(b, oracle.se3_mul(oracle.se3_inverse(a), b)) for a, b in zip(P2, P1)]
    seen = {pa.branch_f32(r) for r in raw}
    assert {(0, False), (1, False), (1, True), (2, False), (2, True), (3, False), (3, True)} <= seen


@pytest.mark.parametrize("batch", BATCHES)
def test_motion_predict_batch_sizes(oracle, hip_ctx, batch):
    P2, P1, want = predict_rows(oracle)
    idx = _spread(len(P1), batch)
    got = _run(hip_ctx, ops.motion_predict_batch, P2[idx], P1[idx], batch, batch + 300)
    assert np.array_equal(_bits(got[:batch]), _bits(want[idx]))
    assert np.all(got[batch:] == PLANT)  # rows past `batch` are not written
    assert np.array_equal(_bits(got[0]), _bits(got[batch - 1]))  # the same pose at two positions


def test_pose_compose_every_case(oracle, hip_ctx):
    P, X, want = compose_rows(oracle)
    got = _run(hip_ctx, ops.pose_compose_batch, P, X, len(P), len(P) + 3)
    bad = [pa.poses()[i]["name"] for i in range(len(P)) if not np.array_equal(_bits(got[i]), _bits(want[i]))]
    assert not bad, (len(bad), bad[:5])
    assert np.all(got[len(P):] == PLANT)


@pytest.mark.parametrize("batch", BATCHES)
def test_pose_compose_batch_sizes(oracle, hip_ctx, batch):
    P, X, want = compose_rows(oracle)
    idx = _spread(len(P), batch)
    got = _run(hip_ctx, ops.pose_compose_batch, P[idx], X[idx], batch, batch + 300)
    assert np.array_equal(_bits(got[:batch]), _bits(want[idx]))
    assert np.all(got[batch:] == PLANT)
    assert np.array_equal(_bits(got[0]), _bits(got[batch - 1]))


def _same_pose(got, want):
    """bit for bit; where the oracle's result holds a NaN, by value (host and device may produce different NaN payloads)"""
    if np.isnan(want).any():
        return np.array_equal(got, want, equal_nan=True)
    return np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("form", [0, 1])
def test_gn_step_every_system(oracle, hip_ctx, variant, form):
    variant(damping_form=form)
    seen = set()
    for s in pa.systems():
        for X0 in (pa.X0, np.eye(4, dtype=f32)):
            want, rc_want = oracle.gn_step(oracle.linear_system(s["H"], s["b"]), s["damping"], X0)
            got, rc = ops.gn_step(hip_ctx, s["H"], s["b"], s["damping"], X0, damping_form=form)
            assert rc == rc_want, (s["name"], rc, rc_want)
            assert _same_pose(got, want), (s["name"], got, want)
            if rc_want:
                assert np.array_equal(_bits(got), _bits(X0)), s["name"]  # a bad pivot leaves X as it was
            seen.add((s["expect"], rc_want))
    assert ("bad_pivot", 1) in seen and ("ok", 0) in seen and ("nan_result", 0) in seen


def test_gn_step_plain_entry_and_unread_upper_triangle(oracle, hip_ctx):
    """prs_gn_step is prs_gn_step_ex with the diagonal form; NaN above the diagonal changes nothing"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    results = {}
    for name in ("clean", "nan_upper_triangle", "negative_pivot_3", "unit_step_2"):
        s = pa.system(name)
        X = np.ascontiguousarray(pa.X0.reshape(16).copy())
        rc = _lib.load().prs_gn_step(hip_ctx._h, p(s["H"]), p(s["b"]), float(s["damping"]), p(X))
        want, rc_want = oracle.gn_step(oracle.linear_system(s["H"], s["b"]), s["damping"], pa.X0)
        assert rc == rc_want and np.array_equal(_bits(X.reshape(4, 4)), _bits(want)), name
        results[name] = X
    assert np.array_equal(_bits(results["clean"]), _bits(results["nan_upper_triangle"]))
    assert np.array_equal(_bits(results["negative_pivot_3"]), _bits(pa.X0.reshape(16)))


def _graph_batch(hip_ctx, lm_workspace):
    cs = list(pa.graphs())
    graphs = ops.PoseGraphBatch(0, len(cs), 2, 1, lm=lm_workspace)
    for b, c in enumerate(cs):
        graphs.upload(b, c["poses"], c["fixed"], (c["src"], c["dst"], c["Z"], c["omega"]))
    return cs, graphs


def test_pose_graph_edge_error_beyond_120_degrees(hip_ctx):
    """t2tnq<double> in linearize_edge: two-node graphs whose edge error at the guess is 2.5 rad about x / y / z, a half turn, and on
    either side of the 120-degree seam (tests/test_pose_algebra_ref.py checks the branch each takes).  Gauss-Newton, 3 iterations;
    whatever status the restatement reports is the expectation"""
    hip_ctx.use_torch_stream()
    cs, graphs = _graph_batch(hip_ctx, False)
    damping, form, eps, iterations = 1e-6, pg.DAMPING_DIAG, 0.0, 3
    P = ops.pose_graph_params(dict(damping=damping, max_iterations=iterations, epsilon=eps), damping_form=form)
    ops.pose_graph_optimize_batch(hip_ctx, P, graphs)
    hip_ctx.synchronize()
    for b, c in enumerate(cs):
        w = pg.optimize(c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], c["omega"], damping, form, iterations, eps)
        assert_same_gn(graphs.poses_of(b), graphs.result_of(b), w, c["name"])


def test_pose_graph_lm_edge_error_beyond_120_degrees(hip_ctx):
    """the same graphs through the Levenberg-Marquardt entry with the shipped icl parameters"""
    hip_ctx.use_torch_stream()
    cs, graphs = _graph_batch(hip_ctx, True)
    rounds, eps = 10, 1e-3
    P = ops.pose_graph_lm_params(configs.get("icl")["graph"], max_iterations=rounds, epsilon=eps)
    ops.pose_graph_optimize_lm_batch(hip_ctx, P, graphs)
    hip_ctx.synchronize()
    for b, c in enumerate(cs):
        w = lm.optimize_lm(c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], c["omega"], {}, rounds, eps)
        assert_same_lm(graphs.poses_of(b), graphs.lm_result_of(b), w, c["name"])
