"""The place bank on the device (prs_place_bank_*: ops.PlaceBank, ops.place_bank_query_batch, ops.BankDetectorBatch) against both of
its references, byte for byte: the numpy restatement (tests/place_bank_ref.py) and the existing prs_place_query_batch /
prs_place_gather_pairs against a PlaceDatabase built with the host add() from that sequence's maps alone -- the bit-parity of the
device append with the host add.  Compared per query: status, index_query, n_candidates, candidates, n_corr, the correspondences'
bytes, match_counts [0, n_maps), best_keys [0, n_rows), the link outputs, and the gathered pair slots' counts and bytes.

Shapes: batch 3, query_stride 272 (two query blocks: rows 255 / 256 / 257 exist), map_stride 5, row_stride 1088 (two database slices).
"""
import ctypes as C

import numpy as np
import pytest

import place_bank_ref as pbr
import place_ref as pr
from place_cases import assert_same, cparams, random_rows
from srrg2_proslam_amd import _lib, configs

pytestmark = pytest.mark.gpu
B, QS, MS, RS, MAXC = 3, 272, 5, 1088, 8
NO_KEY = 0xFFFFFFFF


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


@pytest.fixture(scope="module")
def base():
    """64 random rows every descriptor of these tests is a near-copy of (shared, read only)"""
    return random_rows(np.random.default_rng(2024), 64)


def near(rng, base, n, flips=4):
    """n rows, each a base row with up to `flips` bits flipped: copies of one base row are within 2 * flips bits, others ~128 apart"""
    out = base[rng.integers(0, len(base), n)].copy()
    bits = rng.integers(0, 256, (n, flips))
    for f in range(flips):
        out[np.arange(n), bits[:, f] >> 3] ^= (np.uint8(1) << (bits[:, f] & 7).astype(np.uint8))
    return out


def mask_of(rng, n, k):
    """k Valid rows among n, interleaved with invalid ones"""
    v = np.zeros(n, np.uint8)
    v[rng.permutation(n)[:k]] = 1
    return v


def item(rng, base, gid, n=QS, valid_rows=None, n_query=None, append_n=None):
    n_rows = max(n, 1)
    it = dict(gid=gid, desc=near(rng, base, n_rows)[:n], xyz=rng.integers(-50, 50, (n_rows, 3)).astype(np.float32)[:n],
              valid=None if valid_rows is None else mask_of(rng, n, valid_rows), n_query=n if n_query is None else n_query)
    it["append_n"] = it["n_query"] if append_n is None else append_n
    return it


def params(ops, age=0, max_candidates=MAXC):
    return ops.place_params(dict(maximum_descriptor_distance=30.0, minimum_age_difference_to_candidates=age, relocalize_min_inliers=4),
                            max_candidates=max_candidates)


class PairBuf:
    """the pair slots of a gather (prs_place_pairs), filled with a pattern so that rows the gather must not write show"""

    def __init__(self, slots, fixed_stride, moving_stride):
        import torch
        dev = torch.device("cuda", 0)
        self.fs, self.ms = fixed_stride, moving_stride
        self.fixed_xyz = torch.full((slots, fixed_stride, 4), 7.0, dtype=torch.float32, device=dev)
        self.fixed_desc = torch.full((slots, fixed_stride, 32), 0xAB, dtype=torch.uint8, device=dev)
        self.moving_xyz = torch.full((slots, moving_stride, 4), 7.0, dtype=torch.float32, device=dev)
        self.moving_desc = torch.full((slots, moving_stride, 32), 0xAB, dtype=torch.uint8, device=dev)
        self.n_fixed = torch.full((slots,), -3, dtype=torch.int32, device=dev)
        self.n_moving = torch.full((slots,), -3, dtype=torch.int32, device=dev)
        self.X = torch.zeros((slots, 16), dtype=torch.float32, device=dev)

    def descriptor(self):
        d = _lib.PlacePairs()
        d.fixed_stride, d.moving_stride = self.fs, self.ms
        d.fixed_xyz, d.fixed_desc, d.n_fixed = self.fixed_xyz.data_ptr(), self.fixed_desc.data_ptr(), self.n_fixed.data_ptr()
        d.moving_xyz, d.moving_desc, d.n_moving = self.moving_xyz.data_ptr(), self.moving_desc.data_ptr(), self.n_moving.data_ptr()
        d.X = self.X.data_ptr()
        return d

    def slots_of(self, b, maxc):
        out = []
        for s in range(b * maxc, (b + 1) * maxc):
            nf, nm = int(self.n_fixed[s].item()), int(self.n_moving[s].item())
            out.append(dict(n_fixed=nf, n_moving=nm, fixed_desc=self.fixed_desc[s, :max(nf, 0)].cpu().numpy(),
                            fixed_xyz=self.fixed_xyz[s, :max(nf, 0)].cpu().numpy(), moving_desc=self.moving_desc[s, :max(nm, 0)].cpu().numpy(),
                            moving_xyz=self.moving_xyz[s, :max(nm, 0)].cpu().numpy(), X=self.X[s].cpu().numpy()))
        return out


def snapshot(q, b, maps, rows):
    """every output of query b, as bytes: counts and keys up to the live sizes"""
    nc = int(q.n_candidates[b].item())
    n_corr = q.n_corr[b].cpu().numpy().copy()
    corr = [q.corr[b, k, :n_corr[k]].cpu().numpy().tobytes() for k in range(q.max_candidates)]
    return dict(status=int(q.status[b].item()), index_query=int(q.index_query[b].item()), n_candidates=nc,
                candidates=q.candidates[b].cpu().numpy().tolist(), n_corr=n_corr.tolist(), corr=corr,
                counts=q.match_counts[b, :maps].cpu().numpy().view(np.uint32).tolist(),
                keys=q.best_keys[b, :rows].cpu().numpy().view(np.uint32).tobytes())


def expected_keys(db, P, desc, valid):
    """best_keys [0, rows) of a query from the checker's distances: distance << 23 | query index of the best match, pads and
    unmatched rows ~0"""
    qv = np.arange(len(desc)) if valid is None else np.flatnonzero(valid)
    out = []
    for m in db.maps:
        n = len(m["desc"])
        keys = np.full(pbr.padded(n), NO_KEY, np.int64)
        if n and len(qv):
            d = pr.distances(desc[qv], m["desc"])
            k = np.where(d.astype(np.float32) < np.float32(P["maximum_descriptor_distance"]), (d << 23) | qv[:, None], NO_KEY)
            keys[:n] = k.min(axis=0)
        out.append(keys.astype(np.uint32))
    return np.concatenate(out).tobytes() if out else b""


def same_slots(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["n_fixed"], g["n_moving"]) == (w["n_fixed"], w["n_moving"]), (what, k)
        for f in ("fixed_desc", "fixed_xyz", "moving_desc", "moving_xyz", "X"):
            assert g[f].tobytes() == w[f].tobytes(), (what, k, f)


class Rig:
    """a bank with its query and pair buffers, per sequence a twin PlaceDatabase grown with the host add(), and the numpy bank"""

    def __init__(self, ctx, ops, P, batch=B, query_stride=QS, map_stride=MS, row_stride=RS, base_ids=None, twins=True):
        import torch
        self.ctx, self.ops, self.P, self.B, self.qs = ctx, ops, P, batch, query_stride
        self.bank = ops.PlaceBank(ctx, batch, map_stride, row_stride)
        self.q = ops.PlaceQueries(0, batch, query_stride, P.max_candidates, None, count_stride=map_stride, key_stride=self.bank.row_stride,
                                  corr_stride=min(query_stride, self.bank.row_stride), with_valid=True)
        self.base_ids = base_ids
        self.base_dev = torch.tensor(base_ids, dtype=torch.int64, device=self.q.desc.device) if base_ids is not None else None
        self.links = ops.PlaceBankLinks(0, batch, P.max_candidates, self.base_dev)
        self.pairs = PairBuf(batch * P.max_candidates, query_stride, query_stride)
        self.twins = [ops.PlaceDatabase(ctx) for _ in range(batch)] if twins else None
        self.ref = pbr.Bank(batch, map_stride, row_stride)

    def close(self):
        self.bank.close()
        for t in self.twins or []:
            t.close()

    def upload(self, items):
        q = self.q
        q.valid.fill_(1)
        for b, it in enumerate(items):
            q.upload(b, it["gid"], it["desc"], it["xyz"], it["valid"])
            q.n_query[b] = it["n_query"]

    def launch_query(self):
        self.ops.place_bank_query_batch(self.ctx, self.bank, self.P, self.q, self.links)
        q, p = self.q.descriptor(), self.pairs.descriptor()
        rc = _lib.load().prs_place_bank_gather_pairs(self.bank._h, C.byref(self.P), C.byref(q), C.byref(p))
        assert rc == 0

    def launch_append(self, items):
        for b, it in enumerate(items):
            if it["append_n"] != it["n_query"]:
                self.q.n_query[b] = it["append_n"]
        self.bank.append(self.q, self.base_dev)

    def read(self):
        """the device results of every query: (snapshot, pair slots, link outputs)"""
        maps, rows, _ = self.ref.sizes()
        return [(snapshot(self.q, b, int(maps[b]), int(rows[b])), self.pairs.slots_of(b, self.P.max_candidates),
                 (self.links.candidates_flat[b].cpu().numpy().tolist(), int(self.links.query_node[b].item()))) for b in range(self.B)]

    def check_query(self, items, got, what=""):
        """against the numpy bank and against the twin databases; returns the reference results"""
        P, Pc, maxc, out = self.P, cparams(self.P), self.P.max_candidates, []
        maps, rows, _ = self.ref.sizes()
        for b, it in enumerate(items):
            tag = "%s seq %d" % (what, b)
            snap, slots, (flat, node) = got[b]
            n = it["n_query"]
            want = self.ref.query(b, Pc, it["gid"], it["desc"], it["valid"], n_query=n, query_stride=self.qs)
            out.append(want)
            # ---- the numpy restatement
            as_result = dict(status=snap["status"], candidates=snap["candidates"][: snap["n_candidates"]], counts=snap["counts"],
                             corr=[np.frombuffer(c, pr.CORR_DTYPE) for c in snap["corr"][: snap["n_candidates"]]])
            assert_same(as_result, want, tag)
            assert snap["n_candidates"] == len(want["candidates"]) and snap["candidates"][snap["n_candidates"]:] == [-1] * (maxc - snap["n_candidates"]), tag
            assert snap["index_query"] == want["index_query"], tag
            assert snap["n_corr"] == [len(c) for c in want["corr"]] + [0] * (maxc - len(want["corr"])), tag
            for c, w in zip(snap["corr"], want["corr"]):
                assert c == w.tobytes(), tag
            counted = want["status"] >= 0 and want["status"] != pr.WARN_EMPTY_INPUT or len(want["candidates"]) > 0
            if counted:
                assert snap["counts"] == want["counts"].tolist(), tag
                assert snap["keys"] == expected_keys(self.ref.dbs[b], Pc, it["desc"][:n], None if it["valid"] is None else it["valid"][:n]), tag
            base = 0 if self.base_ids is None else self.base_ids[b]
            assert (flat, node) == self.ref.links(b, want, it["gid"], maxc, base), tag
            ref_slots = pr.gather_pairs(self.ref.dbs[b], want, it["desc"][:max(n, 0)], it["xyz"][:max(n, 0)],
                                        None if it["valid"] is None else it["valid"], maxc)
            for k, (g, w) in enumerate(zip(slots, ref_slots)):
                assert (g["n_fixed"], g["n_moving"]) == (w["n_fixed"], w["n_moving"]), (tag, k)
                assert g["fixed_desc"].tobytes() == w["fixed_desc"].tobytes() and g["moving_desc"].tobytes() == w["moving_desc"].tobytes(), (tag, k)
                assert np.array_equal(g["fixed_xyz"][:, :3], w["fixed_xyz"]) and np.array_equal(g["moving_xyz"][:, :3], w["moving_xyz"]), (tag, k)
                assert not g["moving_xyz"][:, 3].any() and np.array_equal(g["X"].reshape(4, 4), np.eye(4, dtype=np.float32)), (tag, k)
            # ---- prs_place_query_batch + prs_place_gather_pairs against the twin database of this sequence alone
            if self.twins is not None:
                twin = self.twins[b]
                assert twin.size()[:2] == (int(maps[b]), int(rows[b])), tag
                tq = self.ops.PlaceQueries(0, 1, self.qs, maxc, twin, with_valid=True)
                tq.upload(0, it["gid"], it["desc"], it["xyz"], it["valid"])
                tq.n_query[0] = n
                tp = PairBuf(maxc, self.qs, self.qs)
                self.ops.place_query_batch(self.ctx, twin, P, tq)
                d, p = tq.descriptor(), tp.descriptor()
                assert _lib.load().prs_place_gather_pairs(twin._h, C.byref(P), C.byref(d), C.byref(p)) == 0
                self.ctx.synchronize()
                assert snapshot(tq, 0, int(maps[b]), int(rows[b])) == snap, tag + " twin"
                same_slots(slots, tp.slots_of(0, maxc), tag + " twin")
        return out

    def check_append(self, items, what=""):
        """the statuses, the twins and the numpy bank brought in step, sizes and node_of_map"""
        want = self.ref.append([dict(n_query=it["append_n"], graph_id=it["gid"], desc=it["desc"], valid=it["valid"], xyz=it["xyz"])
                                for it in items], query_stride=self.qs, bases=self.base_ids)
        got = self.bank.append_status.cpu().numpy().tolist()
        assert got == want, (what, got, want)
        for b, it in enumerate(items):
            if want[b] == pbr.OK and self.twins is not None:
                n = it["append_n"]
                self.twins[b].add(it["gid"], it["desc"][:n], it["xyz"][:n], None if it["valid"] is None else it["valid"][:n])
        for a, r in zip(self.bank.sizes(), self.ref.sizes()):
            assert np.array_equal(a, r), (what, a, r)
        nodes = self.bank.node_of_map.cpu().numpy()
        for b in range(self.B):
            assert nodes[b].tolist() == self.ref.nodes[b] + [-1] * (self.bank.map_stride - len(self.ref.nodes[b])), what
        return want

    def step(self, items, append=True, what=""):
        self.upload(items)
        self.launch_query()
        self.ctx.synchronize()
        res = self.check_query(items, self.read(), what)
        st = None
        if append:
            self.launch_append(items)
            self.ctx.synchronize()
            st = self.check_append(items, what)
        return res, st


def test_growth_against_both_references(env, base):
    ctx, ops = env
    rng = np.random.default_rng(11)
    rig = Rig(ctx, ops, params(ops))
    valid_rows = [17, 16, 1, 15, 240, 20]
    for s in range(6):
        items = [item(rng, base, 100 + s, valid_rows=valid_rows[s]), item(rng, base, 100 + s), item(rng, base, 100 + s, append_n=0)]
        res, st = rig.step(items, what="step %d" % s)
        assert st[2] == pbr.WARN_EMPTY_INPUT
        assert st[0] == (pbr.OK if s < 5 else pbr.ERR_CAPACITY) and st[1] == (pbr.OK if s < 4 else pbr.ERR_CAPACITY)
        assert res[1]["candidates"] == list(range(min(s, 4))) and not res[2]["candidates"]
    maps, rows, big = rig.bank.sizes()
    assert maps.tolist() == [5, 4, 0] and rows.tolist() == [32 + 16 + 16 + 16 + 240, 1088, 0] and big.tolist() == [240, 272, 0]
    # the refused appends changed nothing: the same queries give the same answers
    res, _ = rig.step([item(rng, base, 200), item(rng, base, 200), item(rng, base, 200)], append=False, what="after refusals")
    assert {0, 1, 3, 4} <= set(res[0]["candidates"])  # (the map of one row has about as many matches as the inlier rule asks)
    assert res[1]["candidates"] == [0, 1, 2, 3]  # the fourth map straddles row 1024
    rig.close()


def test_isolation(env, base):
    ctx, ops = env
    rng = np.random.default_rng(12)
    rig = Rig(ctx, ops, params(ops))
    first = item(rng, base, 5)
    # the same graph id in every sequence: accepted in both that store it
    _, st = rig.step([dict(first), dict(first), dict(first, append_n=0)], what="store")
    assert st == [pbr.OK, pbr.OK, pbr.WARN_EMPTY_INPUT]
    # sequence 2 asks with an exact copy of sequence 1's first map: nothing; sequence 1 with the same rows finds it
    copy = dict(first, gid=6)
    res, st = rig.step([dict(first, append_n=QS), dict(copy, append_n=0), dict(copy, append_n=0)], what="copy")
    assert res[1]["candidates"] == [0] and len(res[1]["corr"][0]) == QS and (res[1]["corr"][0]["response"] == 0).all()
    assert res[2]["candidates"] == [] and res[2]["status"] == 0 and res[2]["index_query"] == 0
    assert not rig.q.match_counts[2].any().item() and not rig.q.n_corr[2].any().item()
    # stored twice in one sequence: refused, nothing changes (check_append compared sizes and nodes)
    assert st == [pbr.ERR_RANGE, pbr.WARN_EMPTY_INPUT, pbr.WARN_EMPTY_INPUT]
    rig.close()


def test_rules_on_own_indices(env, base):
    ctx, ops = env
    rng = np.random.default_rng(13)
    rig = Rig(ctx, ops, params(ops, age=1, max_candidates=2))
    stored = [item(rng, base, 40 + m, n=150 + 50 * m) for m in range(3)]
    for m in range(3):  # sequence 0 holds three maps, sequence 1 one, sequence 2 none
        rig.step([stored[m], dict(stored[m], append_n=stored[m]["n_query"] if m == 0 else 0), dict(stored[m], append_n=0)],
                 what="store %d" % m)
    assert rig.bank.sizes()[0].tolist() == [3, 1, 0]
    q = item(rng, base, 77)
    # a new graph id: index_query 3, map 2 is too young
    res, _ = rig.step([q, q, q], append=False, what="new id")
    assert res[0]["index_query"] == 3 and res[0]["candidates"] == [0, 1] and res[0]["counts"][2] > 4
    assert res[1]["index_query"] == 1 and res[1]["candidates"] == [] and res[2]["index_query"] == 0
    # a re-queried stored id 40 (index 0): the difference wraps for maps 1 and 2, map 0 itself is excluded
    rq = dict(q, gid=40)
    res, _ = rig.step([rq, rq, rq], append=False, what="requery")
    assert res[0]["index_query"] == 0 and res[0]["candidates"] == [1, 2] and res[0]["status"] == 0
    assert res[1]["index_query"] == 0 and res[1]["candidates"] == []  # its only map is the query's own
    # all rows invalid | n_query 0 | a negative graph id
    res, _ = rig.step([dict(q, valid=np.zeros(QS, np.uint8)), dict(q, n_query=0, append_n=0), dict(q, gid=-4)], append=False, what="bad")
    assert [r["status"] for r in res] == [0, pr.WARN_EMPTY_INPUT, pr.ERR_RANGE] and not any(r["candidates"] for r in res)
    # n_query above the slot
    res, _ = rig.step([dict(q, n_query=QS + 1, append_n=0), q, q], append=False, what="over")
    assert res[0]["status"] == pr.ERR_CAPACITY and res[0]["candidates"] == []
    rig.close()
    # more candidates than slots (age 0: all three maps pass, two slots), and the same against an empty bank
    rig = Rig(ctx, ops, params(ops, age=0, max_candidates=2))
    res, _ = rig.step([q, q, q], append=False, what="empty bank")
    assert all(r["status"] == 0 and r["candidates"] == [] and r["index_query"] == 0 for r in res)
    for m in range(3):
        rig.step([stored[m], dict(stored[m], append_n=0), dict(stored[m], append_n=0)], what="store again %d" % m)
    res, _ = rig.step([q, q, q], append=False, what="overflow")
    assert res[0]["status"] == pr.ERR_CAPACITY and res[0]["candidates"] == [0, 1] and rig.read()[0][2][1] == -1
    rig.close()


def test_append_edge_cases(env, base):
    ctx, ops = env
    import torch
    rng = np.random.default_rng(14)
    rig = Rig(ctx, ops, params(ops), base_ids=[2**31, 2**31 + 5, 2**31 + 9])
    a = item(rng, base, 2**31 + 9, n=100)
    # sequence 0 stores a map without a Valid row: 0 rows, never a candidate, index_query advances
    _, st = rig.step([dict(a, valid=np.zeros(100, np.uint8)), a, dict(a, append_n=0)], what="no valid row")
    assert st[:2] == [pbr.OK, pbr.OK] and rig.bank.sizes()[1].tolist() == [0, 112, 0]
    assert int(rig.bank.node_of_map[1, 0].item()) == 4  # (int32) (graph id - base) for ids above 2^31
    res, _ = rig.step([dict(a, gid=2**31 + 10)] * 3, what="after")
    assert res[0]["candidates"] == [] and res[0]["index_query"] == 1 and res[0]["counts"].tolist() == [0] and res[1]["candidates"] == [0]
    # valid = NULL and xyz = NULL: every row is stored, with zero points
    class Slots:  # the leading fields of a query batch, without the optional ones
        pass
    s = Slots()
    s.batch, s.query_stride, s.desc, s.n_query, s.graph_id = B, QS, rig.q.desc, rig.q.n_query, rig.q.graph_id
    bare = item(rng, base, 2**31 + 11, n=33)
    rig.upload([bare] * 3)
    rig.bank.append(s, rig.base_dev)
    ctx.synchronize()
    assert rig.bank.append_status.cpu().numpy().tolist() == [0, 0, 0]
    zero = dict(bare, xyz=np.zeros((33, 3), np.float32))
    rig.ref.append([dict(n_query=33, graph_id=bare["gid"], desc=bare["desc"], valid=None, xyz=None)] * 3, bases=rig.base_ids)
    for t in rig.twins:
        t.add(bare["gid"], bare["desc"], zero["xyz"])
    res, _ = rig.step([dict(bare, gid=2**31 + 12)] * 3, append=False, what="bare")
    assert all(r["candidates"] and r["candidates"][-1] == int(m) - 1 for r, m in zip(res, rig.bank.sizes()[0]))
    # clear(): the bank answers as if new, and an id stored before can be stored again
    rig.bank.clear()
    rig.ref.clear()
    for t in rig.twins:
        t.clear()
    assert all(not x.any() for x in rig.bank.sizes()) and (rig.bank.node_of_map == -1).all().item()
    res, st = rig.step([a] * 3, what="after clear")
    assert st == [pbr.OK] * 3 and all(r["candidates"] == [] and r["index_query"] == 0 for r in res)
    assert isinstance(rig.bank.node_of_map, torch.Tensor)
    rig.close()


def test_captured_step_sees_what_earlier_replays_stored(env, base):
    """query, gather and append captured once: every replay searches the maps the replays before it stored.  prs_place_query_batch
    cannot do this: its launch arguments hold the database's sizes as they were at capture."""
    import torch
    ctx, ops = env
    rng = np.random.default_rng(15)
    P = params(ops)
    cap, eager = Rig(ctx, ops, P, twins=False), Rig(ctx, ops, P)
    idle = [item(rng, base, 1, n_query=0, append_n=0)] * B
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        cap.upload(idle)
        cap.launch_query()  # warm-up on the capture stream (empty slots: nothing is stored)
        cap.launch_append(idle)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cap.launch_query()
            cap.bank.append(cap.q, None)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    torch.cuda.synchronize()
    assert not cap.bank.sizes()[0].any()
    steps = [[item(rng, base, 10 * t + b, n=200 + 36 * b if b == 0 or (t + b) % 3 else 0) for b in range(B)] for t in range(3)]
    again = steps[1][0]  # what sequence 0 stored in the second replay, seen again with a new id and a few more flipped bits
    steps.append([dict(again, gid=90, desc=near(rng, again["desc"], len(again["desc"]), 2)), item(rng, base, 91), item(rng, base, 92)])
    assert again["n_query"] > 0
    for t, items in enumerate(steps):
        cap.upload(items)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = cap.read()
        cap.check_query(items, got, "replay %d" % t)
        cap.check_append(items, "replay %d" % t)
        eager.upload(items)
        eager.launch_query()
        ctx.synchronize()
        twin = eager.read()
        res = eager.check_query(items, twin, "eager %d" % t)
        eager.launch_append(items)
        ctx.synchronize()
        eager.check_append(items, "eager %d" % t)
        for b in range(B):
            assert got[b][0] == twin[b][0] and got[b][2] == twin[b][2], (t, b)
            same_slots(got[b][1], twin[b][1], "replay %d seq %d" % (t, b))
    assert 1 in res[0]["candidates"]  # the fourth step finds the map the second replay stored
    cap.close()
    eager.close()


def test_chain_session_to_closure_edge(env):
    """session split -> hand-over slot -> bank detector -> closure edge, with device tensors only between the session step and the
    appended edge (no sizes(), no copy of the map or of the candidate list)"""
    import torch
    import session_cases as sc
    from srrg2_proslam_amd import synthetic as syn
    ctx, ops = env
    F = np.float32
    k = configs.get("kitti")
    rng = np.random.default_rng(77)
    n, cap = 220, 256
    xyz = np.stack([rng.uniform(-8, 8, n), rng.uniform(-2, 2, n), rng.uniform(3, 25, n)], axis=1).astype(F)
    desc = syn.random_descriptors(rng, n)
    T = sc.rotation([0, 1, 0.2], 0.02)
    T[:3, 3] = [0.3, 0.0, -0.1]
    q_xyz = (xyz.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    q_desc = desc.copy()
    q_desc[np.arange(n), rng.integers(0, 32, n)] ^= np.uint8(1) << rng.integers(0, 8, n).astype(np.uint8)
    P = ops.place_params(k["place"], max_candidates=2, minimum_age_difference_to_candidates=0)
    bf, pa = ops.bruteforce_params(k["loop"]["maximum_descriptor_distance"], 0.9), ops.point_align_params(k["loop"])
    # what LoopDetectorBatch gives against a database that holds the planted map alone
    db = ops.PlaceDatabase(ctx)
    db.add(7, desc, xyz)
    direct = ops.LoopDetectorBatch(0, db, 1, cap, 2, moving_stride=cap)
    direct.upload(0, 8, q_desc, q_xyz)
    direct.run(ctx, P, bf, pa)
    want = direct.result_of(0)
    assert want["candidates"] == [0] and want["accepted"] == [1]
    # two sequences; the bank detector's query slots are the session's hand-over slots
    bank = ops.PlaceBank(ctx, 2, 4, 4 * cap)
    maps, frames = ops.MapBatch(0, 2, cap, 1, 4, 1, 1), ops.AlignFrames(0, 2, 1, 1)
    graphs = ops.PoseGraphBatch(0, 2, 8, 8, envelope_blocks=32)
    base = torch.tensor([7, 20], dtype=torch.int64, device=maps.coords.device)
    det = ops.BankDetectorBatch(0, bank, 2, cap, 2, graph_id_base=base)
    sess = ops.SessionBatch(0, maps, frames, graphs, 4, handover=det.queries, graph_id_base=base)
    sp = ops.session_params(k["split"])
    dev = maps.coords.device
    eye, jump = np.eye(4, dtype=F).reshape(16), sc.translation([0, 0, -11.0]).astype(F).reshape(16)

    def frame(Xs, contents):
        for b, (X, c) in enumerate(zip(Xs, contents)):
            if c is not None:
                maps.coords[b, :n, :3] = torch.from_numpy(c[0]).to(dev)
                maps.desc[b, :n] = torch.from_numpy(c[1]).to(dev)
                maps.n_points[b] = n
            frames.X[b] = torch.from_numpy(X).to(dev)
            frames.result.view(torch.int32)[b, ops.AlignResult.status.offset // 4] = 1
        sess.step(ctx, sp)
        det.run(ctx, P, bf, pa)
        graphs.append_closures(ctx, det.view, *det.node_maps())

    sess.step(ctx, sp)
    frame([jump, eye], [(xyz, desc), None])  # sequence 0 splits and stores the planted map; sequence 1 stays
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in det.node_maps())
    # sequence 0 moves on at the same speed and splits again, sequence 1 splits for the first time: both hand over the perturbed copy
    frame([eye, jump], [(q_xyz, q_desc), (q_xyz, q_desc)])
    ctx.synchronize()
    assert [sess.result_of(b)["reason"] for b in range(2)] == [ops.SESSION_SPLIT_VIEWPOINT] * 2
    assert det.queries.graph_id.cpu().numpy().tolist() == [8, 20] and bank.append_status.cpu().numpy().tolist() == [0, 0]
    got, other = det.result_of(0, 1), det.result_of(1, 0)
    assert got["candidates"] == [0] and got["accepted"] == [1] and got["query_node"] == 1
    assert got["search"]["status"] == want["search"]["status"] and np.array_equal(got["search"]["counts"], want["search"]["counts"])
    for a, b in zip(got["search"]["corr"], want["search"]["corr"]):
        assert a.tobytes() == b.tobytes()
    assert np.asarray(got["poses"][0]).tobytes() == np.asarray(want["poses"][0]).tobytes()
    assert other["candidates"] == [] and other["query_node"] == -1 and other["search"]["status"] == 0
    # exactly one closure edge: graph 0, from the query's node 1 to the stored map's node 0, Z = the aligner's X
    assert graphs.n_appended.cpu().numpy().tolist() == [1, 0] and graphs.append_status.cpu().numpy().tolist() == [0, 0]
    src, dst, Z, _ = graphs.edges_of(0)
    assert len(src) == 3 and (src[-1], dst[-1]) == (1, 0)
    assert Z[-1].astype(F).tobytes() == np.asarray(got["poses"][0], F).tobytes()
    assert len(graphs.edges_of(1)[0]) == 1
    assert bank.sizes()[0].tolist() == [2, 1] and bank.node_of_map.cpu().numpy()[:, :2].tolist() == [[0, 1], [0, -1]]
    bank.close()
    db.close()


def test_call_level_refusals(env, base):
    ctx, ops = env
    import torch
    lib = _lib.load()
    rng = np.random.default_rng(17)
    P = params(ops)
    rig = Rig(ctx, ops, P, twins=False)
    rig.upload([item(rng, base, 3)] * B)
    rig.q.status.fill_(-77)
    rig.bank.append_status.fill_(-77)
    good = rig.q.descriptor()
    pairs = rig.pairs.descriptor()

    def query(d, links=None):
        return lib.prs_place_bank_query_batch(rig.bank._h, C.byref(P), C.byref(d), links)

    def edit(**kw):
        d = rig.q.descriptor()
        for name, v in kw.items():
            setattr(d, name, v)
        return d

    def append(**kw):
        a = _lib.PlaceBankAppend()
        a.batch, a.query_stride, a.desc, a.n_query, a.graph_id = B, QS, good.desc, good.n_query, good.graph_id
        a.status = rig.bank.append_status.data_ptr()
        for name, v in kw.items():
            setattr(a, name, v)
        return lib.prs_place_bank_append_batch(rig.bank._h, C.byref(a))

    assert lib.prs_place_bank_query_batch(rig.bank._h, C.byref(P), None, None) == _lib.ERR_NULL
    assert lib.prs_place_bank_query_batch(rig.bank._h, None, C.byref(good), None) == _lib.ERR_NULL
    assert lib.prs_place_bank_append_batch(rig.bank._h, None) == _lib.ERR_NULL
    assert lib.prs_place_bank_gather_pairs(rig.bank._h, C.byref(P), C.byref(good), None) == _lib.ERR_NULL
    for field in ("desc", "n_query", "graph_id", "status", "best_keys", "corr"):
        assert query(edit(**{field: None})) == _lib.ERR_NULL, field
    for field in ("desc", "n_query", "graph_id", "status"):
        assert append(**{field: None}) == _lib.ERR_NULL, field
    links = _lib.PlaceBankLinks()  # links given, their outputs not
    assert query(good, C.byref(links)) == _lib.ERR_NULL
    assert query(edit(batch=B - 1)) == _lib.ERR_RANGE and append(batch=B + 1) == _lib.ERR_RANGE
    assert lib.prs_place_bank_gather_pairs(rig.bank._h, C.byref(P), C.byref(edit(batch=B + 1)), C.byref(pairs)) == _lib.ERR_RANGE
    assert query(edit(count_stride=MS - 1)) == _lib.ERR_CAPACITY
    assert query(edit(key_stride=RS - 1)) == _lib.ERR_CAPACITY
    for qs in (0, 65537):
        assert query(edit(query_stride=qs)) == _lib.ERR_UNSUPPORTED and append(query_stride=qs) == _lib.ERR_UNSUPPORTED
    assert query(edit(desc=good.desc + 2)) == _lib.ERR_UNSUPPORTED
    assert append(desc=good.desc + 4) == _lib.ERR_UNSUPPORTED and append(xyz=good.xyz + 8) == _lib.ERR_UNSUPPORTED
    assert lib.prs_place_bank_gather_pairs(rig.bank._h, C.byref(P), C.byref(edit(desc=good.desc + 4)), C.byref(pairs)) == _lib.ERR_UNSUPPORTED
    h = C.c_void_p()
    for args in ((0, 1, 16), (65536, 1, 16), (1, 0, 16), (1, 1, 0), (1, 1, (1 << 20) + 1)):
        assert lib.prs_place_bank_create(ctx._h, *args, C.byref(h)) == _lib.ERR_RANGE and not h.value
    # an accepted append of slots of 272 rows makes 272 the least corr_stride and moving_stride (capacities decide, not live sizes)
    assert append() == 0
    assert query(edit(corr_stride=QS - 1)) == _lib.ERR_CAPACITY and query(edit(corr_stride=QS)) == 0
    small = PairBuf(B * MAXC, QS, QS - 1)
    assert lib.prs_place_bank_gather_pairs(rig.bank._h, C.byref(P), C.byref(good), C.byref(small.descriptor())) == _lib.ERR_CAPACITY
    ctx.synchronize()
    # nothing was launched by the refused calls: the one accepted append stored one map per sequence, the one accepted query answered
    assert rig.bank.sizes()[0].tolist() == [1] * B and rig.bank.append_status.cpu().numpy().tolist() == [0] * B
    assert (rig.pairs.n_fixed == -3).all().item() and rig.q.status.cpu().numpy().tolist() == [0] * B
    assert isinstance(rig.q.desc, torch.Tensor)
    rig.close()
