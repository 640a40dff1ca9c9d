"""The world map on the device (ops.WorldMapBatch: prs_world_map_batch_run) against its numpy restatement (tests/world_map_ref.py).
Every output array and, with refresh_state, every state array is compared byte for byte: both sides do the same IEEE operations,
so no tolerance is involved.  Output rows the call must not touch are checked against a sentinel."""
import ctypes as C

import numpy as np
import pytest

import world_map_cases as wc
import world_map_ref as ref
from srrg2_proslam_amd import _lib, ops

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0xA5
ROW_OUTPUTS = ("xyz", "desc", "node", "row", "n_opt")


def _push(t, a):
    import torch
    a = np.ascontiguousarray(a)
    t.copy_(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(t.device).reshape(t.shape))


class Rig:
    """a WorldMapBatch over a MapArchive, a MapBatch and a SessionBatch's graphs, all filled directly from a list of sequences in the
    restatement's layout (no tracking needed)"""

    def __init__(self, ctx, seqs, out_stride, outputs=ops.WorldMapBatch.OPTIONAL):
        self.ctx, self.seqs, self.B = ctx, seqs, len(seqs)
        cap, S, NS = seqs[0]["capacity"], seqs[0]["slot_stride"], seqs[0]["node_stride"]
        self.maps = ops.MapBatch(0, self.B, cap, 0, 1, 1, 1)
        self.frames = ops.AlignFrames(0, self.B, 1, 1)
        self.graphs = ops.PoseGraphBatch(0, self.B, NS, NS, envelope_blocks=4 * NS)
        self.sess = ops.SessionBatch(0, self.maps, self.frames, self.graphs, 1)
        self.arch = ops.MapArchive(0, self.maps, NS, S)
        self.upload()
        self.resize(out_stride, outputs)

    def resize(self, out_stride, outputs=ops.WorldMapBatch.OPTIONAL):
        self.wm = ops.WorldMapBatch(self.sess, self.maps, self.arch, out_stride, outputs)
        self.fill_sentinel()

    def fill_sentinel(self):
        import torch
        wm = self.wm
        for t in (wm.xyz, wm.desc, wm.node, wm.row, wm.n_opt, wm.bounds, wm.n_out, wm.n_total, wm.n_nonfinite, wm.status):
            if t is not None:
                t.view(torch.uint8).fill_(SENTINEL)

    def upload(self):
        q = self.seqs
        stack = lambda f: np.stack([f(s) for s in q])  # noqa: E731
        for name in ("coords", "desc", "n_opt", "inlier", "state"):
            _push(getattr(self.maps, name), stack(lambda s: s["live"][name]))
            _push(getattr(self.arch, name), stack(lambda s: s["slots"][name]))
        _push(self.maps.n_points, np.array([s["live"]["n_points"] for s in q], np.int32))
        _push(self.arch.n_points, stack(lambda s: s["slots"]["n_points"]))
        _push(self.arch.slot_of_node, stack(lambda s: s["slot_of_node"]))
        _push(self.graphs.X, stack(lambda s: s["graph_X"]))
        _push(self.graphs.n_nodes, np.array([s["n_nodes"] for s in q], np.int32))
        _push(self.sess.cur_node, np.array([s["cur_node"] for s in q], np.int32))

    def outputs(self):
        """every output and state array of the device as numpy (uint8 views are taken where bytes are compared)"""
        wm = self.wm
        out = {k: getattr(wm, k).cpu().numpy() for k in ROW_OUTPUTS + ("bounds",) if getattr(wm, k) is not None}
        out.update({k: getattr(wm, k).cpu().numpy() for k in ("n_out", "n_total", "n_nonfinite", "status")})
        out["live_state"], out["slot_state"] = self.maps.state.cpu().numpy(), self.arch.state.cpu().numpy()
        return out

    def check(self, p, count_only=False, what=""):
        """run (or count) and compare every sequence with the restatement; -> the restatement's results"""
        self.upload()
        self.fill_sentinel()
        kw = {k: bool(getattr(p, k)) for k in ("require_inlier", "include_live", "refresh_state")}
        (self.wm.count if count_only else self.wm.run)(self.ctx, p)
        self.ctx.synchronize()
        got = self.outputs()
        want = [ref.world_map(s, ref.params(min_n_opt=p.min_n_opt, **kw), None if count_only else self.wm.out_stride) for s in self.seqs]
        for b, w in enumerate(want):
            tag = (what, b)
            for k in ("n_out", "n_total", "n_nonfinite", "status"):
                assert int(got[k][b]) == w[k], tag + (k, int(got[k][b]), w[k])
            n = w["n_out"]
            for k in ROW_OUTPUTS:
                if k in got:
                    assert got[k][b, :n].tobytes() == np.ascontiguousarray(w[k]).tobytes(), tag + (k,)
                    assert (got[k][b, n:].view(np.uint8) == SENTINEL).all(), tag + (k, "rows behind n_out")
            if "bounds" in got:
                if w["bounds"] is None:
                    assert (got["bounds"][b].view(np.uint8) == SENTINEL).all(), tag + ("bounds untouched",)
                else:
                    assert got["bounds"][b].tobytes() == w["bounds"].tobytes(), tag + ("bounds", got["bounds"][b], w["bounds"])
            assert got["live_state"][b].tobytes() == w["live_state"].tobytes(), tag + ("live state",)
            assert got["slot_state"][b].tobytes() == w["slot_state"].tobytes(), tag + ("archive state",)
        return want


def _batch(capacity, slot_stride, B, seed=0):
    rng = np.random.default_rng(1000 * capacity + 10 * slot_stride + B + seed)
    seqs = [wc.standard_sequence(rng, capacity, slot_stride, with_slot_for_cur=(b % 2 == 0)) for b in range(B)]
    for s in seqs:  # "every second row" through the inlier flag, "only the last row of the last map" through a planted n_opt
        for part in (s["live"], s["slots"]):
            part["inlier"][...] = np.arange(capacity) % 2
        last_node = max(n for n in range(s["n_nodes"]) if s["slot_of_node"][n] >= 0)
        last_slot = int(s["slot_of_node"][last_node])
        s["slots"]["n_opt"][last_slot, int(s["slots"]["n_points"][last_slot]) - 1] = 77
        if last_node == s["cur_node"]:  # then the live map is the last one when it replaces the slot
            s["live"]["n_opt"][s["live"]["n_points"] - 1] = 77
    return seqs


# 515 is a multiple neither of 4 nor of the chunk of 256 rows and takes three chunks
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("slot_stride", [1, 5])
@pytest.mark.parametrize("capacity", [1, 63, 64, 65, 257, 515])
def test_filters_and_shapes(hip_ctx, capacity, slot_stride, B):
    seqs = _batch(capacity, slot_stride, B)
    total_rows = (slot_stride + 1) * capacity
    rig = Rig(hip_ctx, seqs, total_rows + 3)
    for live in (True, False):
        everything = rig.check(ops.world_map_params(include_live=live), what="everything, live %d" % live)
        assert all(w["status"] == ref.PRS_OK for w in everything)
        nothing = rig.check(ops.world_map_params(min_n_opt=100, include_live=live, refresh_state=True), what="nothing")
        assert all(w["n_total"] == 0 for w in nothing)
        rig.check(ops.world_map_params(require_inlier=True, include_live=live), what="every second row")
        last = rig.check(ops.world_map_params(min_n_opt=77, include_live=live), what="the last row of the last map")
        assert all(w["n_total"] == 1 and w["node"][0] == max(n for n in range(s["n_nodes"]) if s["slot_of_node"][n] >= 0)
                   for w, s in zip(last, seqs))
        rig.check(ops.world_map_params(min_n_opt=3, include_live=live, refresh_state=True), what="n_opt >= 3, refreshed")
        rig.check(ops.world_map_params(min_n_opt=2, include_live=live), count_only=True, what="count only")
    if slot_stride == 5 and capacity > 1:
        assert everything[0]["n_total"] > capacity  # more than one map took part


def test_more_nodes_than_a_workgroup_has_threads(hip_ctx):
    """1030 nodes, every one with a slot, in a permuted order: the scan walks two tiles of 1024 nodes and carries the base from one to
    the next, the count's slot-to-node search takes several strides, and the bounds pass more than one"""
    rng = np.random.default_rng(1030)
    NS, cap = 1030, 5
    seqs = []
    for b in range(2):
        son = rng.permutation(NS).astype(np.int32)
        seqs.append(wc.make_sequence(rng, cap, NS, NS, NS - b, 1027 - b, son, rng.integers(0, cap + 1, NS), 3))
    rig = Rig(hip_ctx, seqs, NS * cap)
    want = rig.check(ops.world_map_params(min_n_opt=1, refresh_state=True))
    assert all(w["status"] == ref.PRS_OK and w["n_total"] > 1500 and w["node"][-1] >= 1027 for w in want)
    rig.resize(1500)
    assert all(w["status"] == ref.PRS_ERR_CAPACITY for w in rig.check(ops.world_map_params(include_live=False)))


def _scattered_slots(rng, B, capacity, slot_stride, node_stride):
    """B sequences whose slot_stride slots are named by as many nodes picked from all node_stride, in a permuted order; the other
    nodes have no slot.  Point counts 0 .. capacity with both ends planted; the current node has a slot in sequence 0 and none in 1.
    The last node holds a map with rows: it is the one node whose base takes the totals of every wave of the scan before its own"""
    seqs = []
    for b in range(B):
        nn = node_stride - b
        holders = rng.choice(nn - 1, slot_stride, replace=False)
        holders[3] = nn - 1
        son = np.full(nn, -1, np.int32)
        son[holders] = rng.permutation(slot_stride)
        n_points = rng.integers(0, capacity + 1, slot_stride)
        n_points[son[holders[0]]], n_points[son[holders[1]]], n_points[son[holders[3]]] = 0, capacity, capacity // 2 + 1
        cur = int(holders[2]) if b == 0 else int(np.nonzero(son < 0)[0][nn // 3])
        seqs.append(wc.make_sequence(rng, capacity, slot_stride, node_stride, nn, cur, son, n_points, capacity - 7 * b))
    return seqs


@pytest.mark.parametrize("node_stride,capacity,scan_threads,bounds_threads", [(130, 515, 192, 128), (700, 65, 704, 64)])
def test_scans_between_one_wave_and_sixteen(hip_ctx, node_stride, capacity, scan_threads, bounds_threads):
    """the scan runs roundup64(node_stride) threads and the bounds kernel roundup64(maps * chunks): 130 nodes give 3 waves over one
    tile and 41 maps of 3 chunks give 2 waves; 700 nodes give 11 waves over one partial tile.  The other tests run both at 1 or 16"""
    S = 40
    chunks = -(-capacity // 256)
    assert -(-node_stride // 64) * 64 == scan_threads and -(-(S + 1) * chunks // 64) * 64 == bounds_threads
    seqs = _scattered_slots(np.random.default_rng(node_stride), 2, capacity, S, node_stride)
    rig = Rig(hip_ctx, seqs, (S + 1) * capacity + 3)
    for refresh in (True, False):
        want = rig.check(ops.world_map_params(min_n_opt=1, refresh_state=refresh), what="refresh %d" % refresh)
        for w, s in zip(want, seqs):
            assert w["status"] == ref.PRS_OK and w["bounds"] is not None and w["n_total"] > 4 * capacity
            assert len(set(w["node"].tolist())) >= S - 2 and (np.diff(w["node"]) >= 0).all()  # node order, not slot order
            # rows of the last node, so of the last wave, behind rows of at least two waves before it
            assert w["node"][-1] == s["n_nodes"] - 1 and len(set((w["node"] // 64).tolist())) >= 3
    rig.check(ops.world_map_params(require_inlier=True), count_only=True, what="count only")


def test_more_chunks_than_the_scan_loads_at_once(hip_ctx):
    """capacity 2305: ten chunks of 256 rows a map, the scan takes them eight at a time"""
    seqs = _batch(2305, 1, 2)
    rig = Rig(hip_ctx, seqs, 2 * 2305)
    rig.check(ops.world_map_params(min_n_opt=2, include_live=False))
    seqs[1]["slots"]["n_points"][0] = 2049
    want = rig.check(ops.world_map_params(require_inlier=True, refresh_state=True))
    assert want[1]["n_total"] == 1024 + 1152 and want[1]["row"][1023] == 2047


def test_out_stride_edges_and_count_only(hip_ctx):
    seqs = _batch(65, 5, 3)
    rig = Rig(hip_ctx, seqs, 4)
    p = ops.world_map_params(min_n_opt=1)
    counted = rig.check(p, count_only=True)  # sizes the output: nothing but the counts and the status is written
    n = counted[0]["n_total"]
    assert n > 130 and all(w["status"] == ref.PRS_OK and w["n_out"] == 0 for w in counted)
    for out_stride, status in ((n, ref.PRS_OK), (n - 1, ref.PRS_ERR_CAPACITY), (1, ref.PRS_ERR_CAPACITY), (n + 9, ref.PRS_OK)):
        rig.resize(out_stride)
        got = rig.check(p, what="out_stride %d" % out_stride)
        assert got[0]["status"] == status and got[0]["n_out"] == min(n, out_stride) and got[0]["n_total"] == n
        rig.check(ops.world_map_params(min_n_opt=1, refresh_state=True), what="refreshed, out_stride %d" % out_stride)
    rig.check(ops.world_map_params(refresh_state=True), count_only=True, what="count only, refreshed")


def test_optional_outputs_may_all_be_null(hip_ctx):
    rig = Rig(hip_ctx, _batch(257, 5, 3), 1000, outputs=())
    assert rig.wm.desc is None and rig.wm.bounds is None
    d = rig.wm.descriptor()
    assert d.xyz and not d.desc and not d.node and not d.row and not d.n_opt and not d.bounds
    rig.check(ops.world_map_params(min_n_opt=2))
    cloud = rig.wm.cloud_of(1)
    assert sorted(cloud) == ["bounds", "n_nonfinite", "n_out", "n_total", "status", "xyz"] and cloud["bounds"] is None
    assert cloud["xyz"].shape == (cloud["n_out"], 4)


def test_cloud_of(hip_ctx):
    seqs = _batch(65, 5, 3)
    rig = Rig(hip_ctx, seqs, 60)
    want = rig.check(ops.world_map_params())
    for b in range(3):
        cloud = rig.wm.cloud_of(b)
        for k in ("n_out", "n_total", "n_nonfinite", "status"):
            assert cloud[k] == want[b][k]
        assert cloud["n_out"] == 60 and cloud["status"] == ref.PRS_ERR_CAPACITY
        for k in ROW_OUTPUTS:
            assert cloud[k].tobytes() == np.ascontiguousarray(want[b][k]).tobytes(), k
        assert cloud["bounds"].tobytes() == want[b]["bounds"].tobytes()


def test_rows_that_are_not_finite(hip_ctx):
    seqs = _batch(257, 5, 3)
    rig = Rig(hip_ctx, seqs, 6 * 257)
    p = ops.world_map_params(refresh_state=True)
    clean = rig.check(p)
    s = seqs[1]
    slot = int(s["slot_of_node"][1])  # node 1's map is full
    planted = {(1, 0): np.inf, (1, 63): np.nan, (1, 64): -np.inf, (1, 200): np.nan, (1, 256): np.inf}
    for (node, r), v in planted.items():
        s["slots"]["coords"][slot, r, r % 3] = v
    s["live"]["coords"][5, 1] = np.nan
    s["graph_X"][3][7] = np.inf  # a node pose that is not finite takes its whole map out (node 3's map holds one row)
    dirty = rig.check(p, what="planted")
    assert dirty[1]["n_nonfinite"] == len(planted) + 1 + 1 and dirty[1]["n_total"] == clean[1]["n_total"] - dirty[1]["n_nonfinite"]
    assert dirty[0]["n_nonfinite"] == dirty[2]["n_nonfinite"] == 0
    # the neighbours keep their order: the clean cloud without the planted rows
    gone = {(n, r) for n, r in planted} | {(s["cur_node"], 5), (3, 0)}
    keep = np.array([(int(n), int(r)) not in gone for n, r in zip(clean[1]["node"], clean[1]["row"])])
    assert dirty[1]["node"].tolist() == clean[1]["node"][keep].tolist() and dirty[1]["row"].tolist() == clean[1]["row"][keep].tolist()
    assert dirty[1]["xyz"].tobytes() == clean[1]["xyz"][keep].tobytes()
    # a row that the filter drops anyway does not count
    only = rig.check(ops.world_map_params(min_n_opt=100))
    assert only[1]["n_nonfinite"] == 0


def test_bounds_do_not_depend_on_the_sign_of_zero(hip_ctx):
    seqs = _batch(65, 1, 1)
    s = seqs[0]
    for n in range(s["n_nodes"]):
        X = np.eye(4)
        X[0, 3] = -0.0
        s["graph_X"][n] = X.reshape(16)
    for part in (s["live"], s["slots"]):
        part["coords"][..., 0] = np.where(np.arange(65) % 3 == 0, 0.0, -0.0).astype(F)
        part["coords"][..., 1:3] = -np.abs(part["coords"][..., 1:3]) - F(1)
    rig = Rig(hip_ctx, seqs, 200)
    out = rig.check(ops.world_map_params())[0]
    signs = np.signbit(out["xyz"][:, 0])
    assert signs.any() and not signs.all()
    assert out["bounds"][[0, 3]].tobytes() == np.zeros(2, F).tobytes()


def _break(seqs, cause):
    s = seqs[1]
    if cause == "n_nodes 0":
        s["n_nodes"] = 0
    elif cause == "n_nodes beyond node_stride":
        s["n_nodes"] = s["node_stride"] + 1
    elif cause == "cur_node negative":
        s["cur_node"] = -1
    elif cause == "cur_node at n_nodes":
        s["cur_node"] = s["n_nodes"]
    elif cause == "live n_points beyond capacity":
        s["live"]["n_points"] = s["capacity"] + 1
    elif cause == "live n_points negative":
        s["live"]["n_points"] = -1
    elif cause == "slot beyond slot_stride":
        s["slot_of_node"][0] = s["slot_stride"]
    elif cause == "slot n_points beyond capacity":
        s["slots"]["n_points"][int(s["slot_of_node"][1])] = s["capacity"] + 1
    elif cause == "slot n_points negative":
        s["slots"]["n_points"][int(s["slot_of_node"][1])] = -7
    elif cause == "slot named twice":
        s["slot_of_node"][3] = s["slot_of_node"][0]
    else:
        raise AssertionError(cause)


@pytest.mark.parametrize("cause", ["n_nodes 0", "n_nodes beyond node_stride", "cur_node negative", "cur_node at n_nodes",
                                   "live n_points beyond capacity", "live n_points negative", "slot beyond slot_stride",
                                   "slot n_points beyond capacity", "slot n_points negative", "slot named twice"])
def test_a_refused_sequence_writes_its_status_and_counts_alone(hip_ctx, cause):
    seqs = _batch(65, 5, 3)
    _break(seqs, cause)
    rig = Rig(hip_ctx, seqs, 500)
    want = rig.check(ops.world_map_params(refresh_state=True), what=cause)  # the sentinel and both states are compared in check()
    assert [w["status"] for w in want] == [ref.PRS_OK, ref.PRS_ERR_RANGE, ref.PRS_OK]
    assert want[0]["n_total"] > 65 and want[2]["n_total"] > 65
    counted = rig.check(ops.world_map_params(), count_only=True, what=cause + ", count only")
    assert [w["status"] for w in counted] == [ref.PRS_OK, ref.PRS_ERR_RANGE, ref.PRS_OK]


def test_call_level_refusals_write_nothing(hip_ctx):
    rig = Rig(hip_ctx, _batch(65, 5, 2), 500)
    lib, ctx = _lib.load(), hip_ctx._h
    before = rig.outputs()
    D = lambda: [rig.sess.descriptor(), rig.maps.descriptor(), rig.arch.descriptor(), rig.wm.descriptor()]  # noqa: E731

    def run(d, p=None):
        p = ops.world_map_params(refresh_state=True) if p is None else p
        args = [C.byref(x) if x is not None else None for x in [p] + d]
        return lib.prs_world_map_batch_run(ctx, *args)

    assert run(D()) == 0
    hip_ctx.synchronize()
    rig.upload()
    rig.fill_sentinel()
    for which in range(4):
        d = D()
        d[which] = None
        assert run(d) == -1, which
    for which, field in ((0, "coords"), (0, "desc"), (0, "n_points"), (0, "graph_X"), (0, "n_nodes"), (0, "cur_node"), (1, "n_opt"),
                         (1, "inlier"), (1, "state"), (2, "coords"), (2, "desc"), (2, "n_opt"), (2, "inlier"), (2, "n_points"),
                         (2, "slot_of_node"), (2, "state"), (3, "n_out"), (3, "n_total"), (3, "n_nonfinite"), (3, "status"),
                         (3, "workspace")):
        d = D()
        setattr(d[which], field, None)
        assert run(d) == -1, field
    for which in (1, 2):  # without refresh_state the state arrays are not needed
        d = D()
        d[which].state = None
        assert run(d, ops.world_map_params()) == 0
    hip_ctx.synchronize()
    rig.fill_sentinel()
    for which, field, value in ((1, "batch", 3), (2, "batch", 1), (1, "capacity", 64), (2, "capacity", 66), (2, "node_stride", 9),
                                (2, "slot_stride", 0), (0, "batch", 0), (3, "out_stride", -1), (3, "out_stride", 0)):
        d = D()
        setattr(d[which], field, value)
        assert run(d) == ref.PRS_ERR_RANGE, (field, value)
    d = D()
    d[3].xyz, d[3].out_stride = None, 0  # legal in a count-only call
    assert run(d, ops.world_map_params()) == 0
    hip_ctx.synchronize()
    rig.fill_sentinel()
    for which, field, step in ((3, "xyz", 8), (3, "desc", 8), (3, "workspace", 8), (0, "coords", 4), (0, "desc", 8), (2, "coords", 8),
                               (2, "state", 4), (1, "state", 8), (0, "graph_X", 4), (1, "n_opt", 2), (2, "slot_of_node", 1),
                               (3, "node", 2), (3, "bounds", 1), (3, "n_total", 2)):
        d = D()
        setattr(d[which], field, getattr(d[which], field) + step)
        assert run(d) == -5, field
    hip_ctx.synchronize()
    after = rig.outputs()
    for k in ROW_OUTPUTS + ("bounds", "n_out", "n_total", "n_nonfinite", "status"):
        assert (after[k].view(np.uint8) == SENTINEL).all(), k
    for k in ("live_state", "slot_state"):
        assert after[k].tobytes() == before[k].tobytes(), k


def _snapshot(rig, b):
    got = rig.outputs()
    return {k: v[b].tobytes() for k, v in got.items()}


def test_a_sequence_does_not_depend_on_its_batch_or_on_the_run(hip_ctx):
    seqs = _batch(515, 5, 3, seed=5)
    p = ops.world_map_params(min_n_opt=1, refresh_state=True)
    rig3 = Rig(hip_ctx, seqs, 2000)
    rig3.check(p)
    first = _snapshot(rig3, 2)
    rig3.check(p)
    assert _snapshot(rig3, 2) == first  # two runs
    rig1 = Rig(hip_ctx, [seqs[2]], 2000)
    rig1.check(p)
    assert _snapshot(rig1, 0) == first  # position 0 of B = 1 against position 2 of B = 3


def test_captured_graph_replayed_after_the_inputs_change(hip_ctx):
    import torch
    ctx = hip_ctx
    seqs = _batch(257, 5, 3, seed=9)
    rig = Rig(ctx, seqs, 1600)
    p = ops.world_map_params(min_n_opt=1, refresh_state=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        rig.wm.run(ctx, p)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rig.wm.run(ctx, p)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    for replay in range(2):
        for q in seqs:  # the optimiser moves the nodes, the maps grow or shrink, the session moves on
            q["graph_X"][...] = np.stack([wc.rigid(rng) for _ in range(q["node_stride"])])
            q["live"]["n_points"] = int(rng.integers(0, 258))
            q["cur_node"] = (q["cur_node"] + 1 + replay) % q["n_nodes"]
        rig.upload()
        rig.fill_sentinel()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = rig.outputs()
        for b, q in enumerate(seqs):
            w = ref.world_map(q, ref.params(min_n_opt=1, refresh_state=True), 1600)
            assert w["status"] == ref.PRS_OK and int(got["n_total"][b]) == w["n_total"] and int(got["status"][b]) == w["status"]
            for k in ROW_OUTPUTS:
                assert got[k][b, :w["n_out"]].tobytes() == np.ascontiguousarray(w[k]).tobytes(), (replay, b, k)
            assert got["bounds"][b].tobytes() == w["bounds"].tobytes()
            assert got["slot_state"][b].tobytes() == w["slot_state"].tobytes() and got["live_state"][b].tobytes() == w["live_state"].tobytes()


def test_maps_archived_by_the_session_itself(hip_ctx):
    """a real chain: ReentryBatch.step archives two finished maps per sequence, the graph is then moved as an optimiser would move it,
    and the cloud is compared with the restatement fed from MapArchive.slot_of, the route the call replaces"""
    from test_reentry_gpu import Rig as ReentryRig, _walk
    rr_rig = ReentryRig(hip_ctx, 2, 6, 40, 4, 6, handover_stride=40, slot_stride=3, max_measurements=2)
    _walk(rr_rig, np.random.default_rng(11))
    assert rr_rig.arch.n_slots.tolist() == [2, 2] and rr_rig.sess.cur_node.tolist() == [2, 2]
    rng = np.random.default_rng(12)
    X = rr_rig.graphs.X.cpu().numpy().reshape(2, -1, 4, 4).copy()
    for b in range(2):
        for n in range(3):
            X[b, n] = X[b, n] @ np.linalg.inv(np.asarray(wc.rigid(rng, scale=0.05)).reshape(4, 4))
    _push(rr_rig.graphs.X, X.reshape(rr_rig.graphs.X.shape))
    rr_rig.maps.n_points.fill_(7)  # the map the walk ended in has grown since its split
    wm = ops.WorldMapBatch(rr_rig.sess, rr_rig.maps, rr_rig.arch, 200)
    p = dict(min_n_opt=2, require_inlier=True)
    wm.run(hip_ctx, ops.world_map_params(**p))
    hip_ctx.synchronize()
    for b in range(2):
        archived = [(n, rr_rig.arch.slot_of(b, n)) for n in range(2)]
        assert all(m is not None and m["n_points"] > 0 for _, m in archived)
        live = (2, dict(coords=rr_rig.maps.coords[b].cpu().numpy(), n_opt=rr_rig.maps.n_opt[b].cpu().numpy(),
                        inlier=rr_rig.maps.inlier[b].cpu().numpy(), n_points=int(rr_rig.maps.n_points[b].item())))
        want = ref.host_route(archived, live, X[b].reshape(-1, 16), ref.params(**p))
        cloud = wm.cloud_of(b)
        assert cloud["status"] == ref.PRS_OK and cloud["n_out"] == cloud["n_total"] == want.shape[0] and want.shape[0] > 3
        assert cloud["xyz"].tobytes() == want.tobytes()
        assert set(cloud["node"].tolist()) <= {0, 1, 2} and (np.diff(cloud["node"]) >= 0).all()
    rr_rig.close()
