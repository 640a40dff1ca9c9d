"""The pose-graph optimiser on the device (prs_pose_graph_optimize_batch / prs_pose_graph_optimize / prs_pose_graph_append_closures /
the C++ adapter) equals its float64 restatement (tests/pose_graph_ref.py optimize) bit for bit -- poses, chi history, iteration
count, envelope size, status -- for every case of tests/pose_graph_cases.py, both damping forms, the criterion on and off, at any
position of a batch and through either entry point; the status rules of the header; closures appended from a real detector run."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import point_align_ref as par
import pose_graph_cases as pc
import pose_graph_ref as ref
from srrg2_proslam_amd import _lib, configs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(1e-6, ref.DAMPING_DIAG, 1e-3), (1e-6, ref.DAMPING_DIAG, 0.0), (1e-3, ref.DAMPING_IDENTITY, 1e-3), (0.0, ref.DAMPING_IDENTITY, 0.0)]
ITERATIONS = 6


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import ops
    assert torch.cuda.is_available()
    ctx = ops.Context(0)
    yield ctx, ops
    ctx.close()


def params(ops, damping, form, eps, iterations=ITERATIONS, **kw):
    return ops.pose_graph_params(dict(damping=damping, max_iterations=iterations, epsilon=eps), damping_form=form, **kw)


_wanted = {}


def want(c, damping, form, eps, iterations=ITERATIONS, **caps):
    key = (c["name"], damping, form, eps, iterations, tuple(sorted(caps.items())))
    if key not in _wanted:
        _wanted[key] = ref.optimize(c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], c["omega"], damping, form, iterations, eps, **caps)
    return _wanted[key]


def bits(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def assert_same(got_X, got, w, what):
    assert got["status"] == w["status"], (what, got["status"], w["status"])
    assert got["envelope_blocks"] == w["envelope_blocks"] and got["iterations"] == w["iterations"], (what, got, w["iterations"])
    assert got["linearizations"] == len(w["chi"]), what
    assert np.array_equal(bits(got["chi"]), bits(w["chi"])), (what, got["chi"], w["chi"])
    assert np.array_equal(bits(got["chi_final"]), bits(w["chi_final"])), (what, got["chi_final"], w["chi_final"])
    assert np.array_equal(bits(got_X), bits(w["X"])), (what, np.abs(np.asarray(got_X).reshape(-1, 16) - w["X"]).max())


def upload(graphs, b, c):
    graphs.upload(b, c["poses"], c["fixed"], (c["src"], c["dst"], c["Z"], c["omega"]))


def run_batch(ctx, ops, cs, P, node_stride=None, edge_stride=None, envelope_blocks=None):
    ns = node_stride or max(max(len(c["poses"]) for c in cs), 1)
    es = edge_stride or max(max(len(c["src"]) for c in cs), 1)
    graphs = ops.PoseGraphBatch(0, len(cs), ns, es, envelope_blocks)
    for b, c in enumerate(cs):
        upload(graphs, b, c)
    ops.pose_graph_optimize_batch(ctx, P, graphs)
    ctx.synchronize()
    return graphs


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
def test_every_case_equals_the_restatement(env, variant):
    ctx, ops = env
    damping, form, eps = VARIANTS[variant]
    cs = list(pc.cases()) + ([pc.kitti_case()] if variant == 0 else [])
    graphs = run_batch(ctx, ops, cs, params(ops, damping, form, eps))
    for b, c in enumerate(cs):
        assert_same(graphs.poses_of(b), graphs.result_of(b), want(c, damping, form, eps), c["name"])


def test_position_in_the_batch_and_entry_point(env):
    ctx, ops = env
    damping, form, eps = VARIANTS[0]
    P = params(ops, damping, form, eps)
    cs = [pc.case(n) for n in pc.MIXED_BATCH]
    graphs = run_batch(ctx, ops, cs, P)
    for b, c in enumerate(cs):
        assert_same(graphs.poses_of(b), graphs.result_of(b), want(c, damping, form, eps), "mixed %d %s" % (b, c["name"]))
    assert np.array_equal(bits(graphs.poses_of(0)), bits(graphs.poses_of(4)))
    assert np.array_equal(bits(graphs.result_of(0)["chi"]), bits(graphs.result_of(4)["chi"]))
    for c in (pc.case("ring8"), pc.case("omega"), pc.case("n65"), pc.case("n1")):
        X, res, rc = ops.pose_graph_optimize(ctx, P, c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], c["omega"])
        assert rc == 0
        assert_same(X, res, want(c, damping, form, eps), "host entry " + c["name"])


def test_wide_rows_are_factorised_in_place_with_the_same_bits(env):
    """node_stride 1024 leaves the LDS row buffer 194 blocks: n130's closure (1, 129) fits, so force the in-place path through a
    graph whose closure spans more: 200 nodes, closure (0, 199)"""
    ctx, ops = env
    rng = np.random.default_rng(5)
    c = pc._graph("n200", rng, 200, closures=[(0, 199)], noise=(0.02, 0.004))
    damping, form, eps = VARIANTS[0]
    P = params(ops, damping, form, eps, iterations=2)
    w = want(c, damping, form, eps, iterations=2)
    small = run_batch(ctx, ops, [c], P)
    assert_same(small.poses_of(0), small.result_of(0), w, "n200 row in LDS")
    big = run_batch(ctx, ops, [c], P, node_stride=1024, envelope_blocks=w["envelope_blocks"])
    assert_same(big.poses_of(0), big.result_of(0), w, "n200 row in place")


def _status_case(base, **kw):
    c = dict(pc.case(base))
    c.update(kw)
    return c


def test_status_rules(env):
    ctx, ops = env
    import torch
    damping, form, eps = VARIANTS[1]
    P = params(ops, damping, form, eps, iterations=3)
    ring, chain = pc.case("ring8"), pc.case("chain3")
    bad_end = _status_case("chain3", name="bad_endpoint", dst=np.array([1, 3], np.int32))
    self_edge = _status_case("chain3", name="self_edge", dst=np.array([1, 1], np.int32))
    no_free = _status_case("chain3", name="no_free", fixed=np.ones(3, np.uint8))
    no_edges = _status_case("chain3", name="no_edges", src=np.zeros(0, np.int32), dst=np.zeros(0, np.int32), Z=np.zeros((0, 16), np.float32))
    lonely = _status_case("chain3", name="free_node_without_edge", src=np.array([0], np.int32), dst=np.array([1], np.int32),
                          Z=pc.case("chain3")["Z"][:1])
    cs = [ring, bad_end, self_edge, no_free, ring, no_edges, lonely, chain]
    graphs = ops.PoseGraphBatch(0, len(cs) + 5, 8, 8, 21)  # room for ring8 exactly: 21 blocks
    for b, c in enumerate(cs):
        upload(graphs, b, c)
    n = len(cs)
    upload(graphs, n, chain)      # n_nodes > node_stride
    upload(graphs, n + 1, chain)  # n_edges > edge_stride
    upload(graphs, n + 2, chain)  # negative node count
    upload(graphs, n + 3, chain)  # negative edge count
    # n + 4 stays empty: n_nodes == 0
    graphs.n_nodes[n], graphs.n_edges[n + 1], graphs.n_nodes[n + 2], graphs.n_edges[n + 3] = 9, 9, -1, -1
    before = graphs.X.clone()
    ops.pose_graph_optimize_batch(ctx, P, graphs)
    ctx.synchronize()
    got = [graphs.result_of(b) for b in range(n + 5)]
    assert [g["status"] for g in got] == [0, ref.ERR_RANGE, ref.ERR_RANGE, 0, 0, 0, ref.ERR_NOT_POSITIVE, 0, ref.ERR_CAPACITY, ref.ERR_CAPACITY,
                                          ref.ERR_RANGE, ref.ERR_RANGE, ref.WARN_EMPTY_INPUT]
    # the good graphs next to the failing ones are what they are alone
    for b in (0, 4, 7):
        assert_same(graphs.poses_of(b), got[b], want(cs[b], damping, form, eps, iterations=3), "neighbour %d" % b)
    # refused and failed graphs keep their poses; no edges / no free node: success, 0 iterations
    for b in (1, 2, 3, 5, 6, n, n + 1, n + 2, n + 3, n + 4):
        assert torch.equal(graphs.X[b], before[b]), b
        assert got[b]["iterations"] == 0
    assert got[3]["linearizations"] == 0 and np.array_equal(bits(got[3]["chi_final"]), bits(want(no_free, damping, form, eps, iterations=3)["chi_final"]))
    assert got[5]["chi_final"] == 0.0 and got[5]["envelope_blocks"] == 3
    # damping 0 and a free node no edge reaches: its pivot is exactly 0 -- a numeric failure at the first solve
    assert got[6]["linearizations"] == 1 and got[6]["iterations"] == 0
    assert_same(graphs.poses_of(6), got[6], want(lonely, damping, form, eps, iterations=3), "lonely")
    # a workspace of exactly the needed size, and one block short
    for blocks, status in ((21, 0), (20, ref.ERR_CAPACITY)):
        g1 = run_batch(ctx, ops, [ring, chain], P, envelope_blocks=blocks)
        assert [g1.result_of(0)["status"], g1.result_of(1)["status"]] == [status, 0]
        w = want(ring, damping, form, eps, iterations=3, capacity_blocks=blocks)
        assert_same(g1.poses_of(0), g1.result_of(0), w, "workspace of %d blocks" % blocks)
    # call-level refusals
    with pytest.raises(_lib.ProslamHipError) as e:
        ops.pose_graph_optimize_batch(ctx, P, ops.PoseGraphBatch(0, 1, 1025, 4, 8))
    assert e.value.status == _lib.ERR_CAPACITY
    with pytest.raises(_lib.ProslamHipError):
        ops.pose_graph_optimize_batch(ctx, params(ops, 0.0, 0, 0.0, iterations=33), graphs)


def test_captured_graph_replay(env):
    import torch
    ctx, ops = env
    damping, form, eps = VARIANTS[0]
    P = params(ops, damping, form, eps)
    c = pc.case("two_closures_one_row")
    graphs = ops.PoseGraphBatch(0, 1, len(c["poses"]), len(c["src"]))
    upload(graphs, 0, c)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        ops.pose_graph_optimize_batch(ctx, P, graphs)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ops.pose_graph_optimize_batch(ctx, P, graphs)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    upload(graphs, 0, c)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_same(graphs.poses_of(0), graphs.result_of(0), want(c, damping, form, eps), "replay")


def test_closures_from_the_detector(env):
    """KITTI: map 0 = city 00 (node 0); queries city 00 again (node 1) and city 01 (node 2) are accepted, highway 274 (node 3) has no
    candidate.  Slots 0 and 2 of the detector become the edges 1 -> 0 and 2 -> 0 with Z = the aligner's X (movingInFixed with the query
    fixed: X_query^-1 X_candidate), in slot order, behind the three odometry edges; then the graph is optimised; nothing waits for
    the host before the final read."""
    import torch
    from test_ref_pins import OracleBackend
    ctx, ops = env
    B = OracleBackend()
    sc = {s["name"]: s for s in par.scenarios(B)}
    k = configs.get("kitti")
    db = ops.PlaceDatabase(ctx)
    s0 = sc["kitti_00_00"]
    db.add(0, s0["moving_desc"], s0["moving"])
    Pp = ops.place_params(k["place"], max_candidates=2, minimum_age_difference_to_candidates=0)
    unrelated = [u for u in par.unrelated(B) if u["config"] == "kitti"]
    qs = [sc["kitti_00_00"], sc["kitti_00_01"]]
    det = ops.LoopDetectorBatch(0, db, 3, max(len(q["fixed"]) for q in qs + unrelated[:1]), 2)
    for b, q in enumerate(qs):
        det.upload(b, 1 + b, q["fixed_desc"], q["fixed"])
    det.upload(2, 9, unrelated[0]["fixed_desc"], unrelated[0]["fixed"])
    # graph 0: four nodes on a line, 0.8 m apart, odometry that says 0.8 m; graph 1 receives nothing; graph 2 has no room
    step = np.eye(4)
    step[2, 3] = 0.8
    poses = np.stack([np.linalg.matrix_power(step, i) for i in range(4)])
    odo = (np.array([0, 1, 2], np.int32), np.array([1, 2, 3], np.int32), np.stack([step] * 3).astype(np.float32), None)
    fixed = np.array([1, 0, 0, 0], np.uint8)
    graphs = ops.PoseGraphBatch(0, 3, 4, 5)
    small = ops.PoseGraphBatch(0, 1, 4, 4)
    for b in range(3):
        graphs.upload(b, poses, fixed, odo)
    small.upload(0, poses, fixed, odo)
    dev = graphs.X.device
    to_dev = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)
    graph_of_query, node_of_query, node_of_map = to_dev([0, 0, 0]), to_dev([1, 2, 3]), to_dev([0])
    P = params(ops, 1e-6, ref.DAMPING_DIAG, 1e-3, closure_information=4.0)
    torch.cuda.synchronize()
    det.run(ctx, Pp, ops.bruteforce_params(k["loop"]["maximum_descriptor_distance"], 0.9), ops.point_align_params(k["loop"]))
    graphs.append_closures(ctx, det, graph_of_query, node_of_query, node_of_map, P)
    small.append_closures(ctx, det, graph_of_query, node_of_query, node_of_map, P)
    ops.pose_graph_optimize_batch(ctx, P, graphs)
    ctx.synchronize()
    assert [det.result_of(b)["accepted"] for b in range(3)] == [[1], [1], []]
    assert graphs.append_status.tolist() == [0, 0, 0] and graphs.n_appended.tolist() == [2, 0, 0] and graphs.n_edges.tolist() == [5, 3, 3]
    src, dst, Z, om = graphs.edges_of(0)
    assert src.tolist() == [0, 1, 2, 1, 2] and dst.tolist() == [1, 2, 3, 0, 0]
    for e, slot in ((3, 0), (4, 2)):
        assert np.array_equal(Z[e], det.closures.pairs.X_of(slot))
        assert np.array_equal(om[e], 4.0 * np.eye(6, dtype=np.float32))
    # the direction: the aligner registers the candidate's points (moving) in the query's frame (fixed)
    assert (np.abs(par.pose_error(Z[4], qs[1]["truth"])) < np.asarray(qs[1]["bounds"])).all()
    w = ref.optimize(poses.reshape(-1, 16), fixed, src, dst, Z.reshape(-1, 16), om.reshape(-1, 36), 1e-6, ref.DAMPING_DIAG, ITERATIONS, 1e-3)
    assert_same(graphs.poses_of(0), graphs.result_of(0), w, "graph with closures")
    assert w["iterations"] > 0 and w["chi_final"] < w["chi"][0]
    # overflow: 3 + 2 edges do not fit edge_stride 4 -- nothing is appended
    assert small.append_status.tolist() == [ref.ERR_CAPACITY] and small.n_edges.tolist() == [3] and small.n_appended.tolist() == [0]
    # a map without a node is skipped
    graphs.append_closures(ctx, det, to_dev([1, 1, 1]), node_of_query, to_dev([-1]), P)
    ctx.synchronize()
    assert graphs.n_edges.tolist() == [5, 3, 3] and graphs.append_status.tolist() == [0, 0, 0]


def test_plugin_adapter(env):
    exe = os.path.join(ROOT, "tests", "cpp", "test_pose_graph_plugin")
    assert os.path.exists(exe), "build() did not produce the adapter test program"
    c = pc.case("two_closures_one_row")
    tmp = tempfile.mkdtemp()
    names = {n: os.path.join(tmp, "pose_graph_plugin_%s.bin" % n) for n in ("poses", "fixed", "src", "dst", "Z", "out")}
    c["poses"].astype(np.float64).tofile(names["poses"])
    c["fixed"].astype(np.uint8).tofile(names["fixed"])
    c["src"].astype(np.int32).tofile(names["src"])
    c["dst"].astype(np.int32).tofile(names["dst"])
    c["Z"].astype(np.float32).tofile(names["Z"])
    out = subprocess.run([exe, str(len(c["poses"])), str(len(c["src"])), names["poses"], names["fixed"], names["src"], names["dst"], names["Z"],
                          names["out"]], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    w = want(c, 1e-6, ref.DAMPING_DIAG, 1e-3, iterations=10)
    assert "iterations %d" % w["iterations"] in out.stdout
    assert np.array_equal(bits(np.fromfile(names["out"], np.float64)), bits(w["X"]))
