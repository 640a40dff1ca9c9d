"""The place bank without a GPU: its C-ABI (exported entries, struct sizes, offsets, unchanged version) and the numpy restatement
(tests/place_bank_ref.py): the append rules and that a per-sequence query equals B independent place_ref.Database objects."""
import ctypes as C

import numpy as np

import place_bank_ref as pbr
import place_ref as pr
from place_cases import assert_same, flip, pick, random_rows
from srrg2_proslam_amd import _lib

ENTRIES = ("prs_place_bank_create", "prs_place_bank_destroy", "prs_place_bank_clear", "prs_place_bank_sizes", "prs_place_bank_struct_sizes",
           "prs_place_bank_bind_node_of_map", "prs_place_bank_append_batch", "prs_place_bank_query_batch", "prs_place_bank_gather_pairs")


def test_entries_are_exported_and_the_version_stays():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert lib.prs_version() == 104 == _lib.ABI_VERSION


def test_struct_sizes_and_offsets():
    sizes = (C.c_uint64 * 2)()
    _lib.load().prs_place_bank_struct_sizes(sizes)
    assert list(sizes) == [C.sizeof(_lib.PlaceBankAppend), C.sizeof(_lib.PlaceBankLinks)]
    a, q = _lib.PlaceBankAppend, _lib.PlaceQueries
    # two int32, then seven pointers
    assert C.sizeof(a) == 8 + 7 * 8 and C.sizeof(_lib.PlaceBankLinks) == 24
    assert (a.batch.offset, a.query_stride.offset, a.desc.offset, a.graph_id_base.offset, a.status.offset) == (0, 4, 8, 48, 56)
    # the leading fields are those of prs_place_queries, so that a query batch can be stored as it stands
    for f in ("batch", "query_stride", "desc", "valid", "xyz", "n_query", "graph_id"):
        assert getattr(a, f).offset == getattr(q, f).offset, f
    k = _lib.PlaceBankLinks
    assert (k.candidates_flat.offset, k.query_node.offset, k.graph_id_base.offset) == (0, 8, 16)


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    assert lib.prs_place_bank_clear(None) == _lib.ERR_NULL
    assert lib.prs_place_bank_append_batch(None, None) == _lib.ERR_NULL
    assert lib.prs_place_bank_query_batch(None, None, None, None) == _lib.ERR_NULL
    assert lib.prs_place_bank_gather_pairs(None, None, None, None) == _lib.ERR_NULL
    assert lib.prs_place_bank_create(None, 1, 1, 16, None) == _lib.ERR_NULL
    assert lib.prs_place_bank_destroy(None) == 0


def item(rng, n, gid, valid=None):
    return dict(n_query=n, graph_id=gid, desc=random_rows(rng, max(n, 1)), valid=valid,
                xyz=rng.integers(-50, 50, (max(n, 1), 3)).astype(np.float32))


def test_append_pads_to_16_and_keeps_point_order():
    rng = np.random.default_rng(1)
    bank = pbr.Bank(1, 4, 100)
    assert bank.row_stride == 112
    v = (np.arange(40) % 3 != 1).astype(np.uint8)  # 27 Valid rows
    a, b = item(rng, 40, 5, v), item(rng, 16, 9)
    assert bank.append([a]) == [pbr.OK] and bank.append([b]) == [pbr.OK]
    maps, rows, big = bank.sizes()
    assert (maps[0], rows[0], big[0]) == (2, 32 + 16, 27)
    lay = bank.layout(0)
    keep = np.flatnonzero(v)
    assert lay["map_off"] == [0, 32] and lay["map_rows"] == [27, 16] and lay["map_gid"] == [5, 9] and lay["node_of_map"] == [5, 9]
    assert np.array_equal(lay["row_pidx"][:27], keep) and (lay["row_pidx"][27:32] == -1).all()
    assert np.array_equal(lay["desc"][:27], a["desc"][keep]) and not lay["desc"][27:32].any()
    assert np.array_equal(lay["xyz"][:27, :3], a["xyz"][keep]) and not lay["xyz"][:, 3].any() and not lay["xyz"][27:32].any()
    assert lay["tile_map"].tolist() == [0, 0, 1]


def test_empty_but_stored_map_and_no_split():
    rng = np.random.default_rng(2)
    bank = pbr.Bank(2, 3, 64)
    none = item(rng, 10, 7, np.zeros(10, np.uint8))
    assert bank.append([none, item(rng, 0, 7)]) == [pbr.OK, pbr.WARN_EMPTY_INPUT]
    maps, rows, big = bank.sizes()
    assert maps.tolist() == [1, 0] and rows.tolist() == [0, 0] and big.tolist() == [0, 0]
    # the empty map is never a candidate, and it advances index_query
    q = random_rows(rng, 12)
    r = bank.query(0, pr.params(256.5, 0, 0), 8, q)
    assert r["candidates"] == [] and r["index_query"] == 1 and r["counts"].tolist() == [0]
    assert bank.query(1, pr.params(256.5, 0, 0), 8, q)["index_query"] == 0


def test_duplicate_is_per_sequence_and_the_bad_inputs():
    rng = np.random.default_rng(3)
    bank = pbr.Bank(2, 4, 256)
    assert bank.append([item(rng, 20, 11), item(rng, 20, 11)]) == [pbr.OK, pbr.OK]
    before = bank.sizes()
    assert bank.append([item(rng, 20, 11), item(rng, 20, 12)]) == [pbr.ERR_RANGE, pbr.OK]
    assert bank.sizes()[0].tolist() == [1, 2] and bank.sizes()[1][0] == before[1][0]
    assert bank.append([item(rng, -1, 3), item(rng, 5, -2)]) == [pbr.ERR_RANGE, pbr.ERR_RANGE]
    assert bank.append([item(rng, 21, 3), item(rng, 0, -2)], query_stride=20) == [pbr.ERR_CAPACITY, pbr.WARN_EMPTY_INPUT]
    assert bank.sizes()[0].tolist() == [1, 2]
    assert bank.append([item(rng, 5, 2**31 + 7), item(rng, 0, 0)], bases=[2**31, 0])[0] == pbr.OK and bank.nodes[0] == [11, 7]


def test_both_capacity_refusals_leave_the_state():
    rng = np.random.default_rng(4)
    bank = pbr.Bank(2, 2, 48)
    assert bank.append([item(rng, 17, 0), item(rng, 3, 0)]) == [pbr.OK, pbr.OK]      # 32 rows | 16 rows
    assert bank.append([item(rng, 17, 1), item(rng, 3, 1)]) == [pbr.ERR_CAPACITY, pbr.OK]  # rows: 32 + 32 > 48
    assert bank.append([item(rng, 16, 1), item(rng, 1, 2)]) == [pbr.OK, pbr.ERR_CAPACITY]  # fills exactly | maps: 2 == map_stride
    maps, rows, _ = bank.sizes()
    assert maps.tolist() == [2, 2] and rows.tolist() == [48, 32]
    lay = bank.layout(1)
    assert lay["map_gid"] == [0, 1] and lay["map_off"] == [0, 16]
    bank.clear()
    assert bank.sizes()[0].tolist() == [0, 0] and bank.append([item(rng, 17, 0), item(rng, 3, 0)]) == [pbr.OK, pbr.OK]


def test_queries_equal_independent_databases():
    rng = np.random.default_rng(5)
    B, P = 3, pr.params(30.0, 1, 2)
    bank, dbs = pbr.Bank(B, 6, 2048), [pr.Database() for _ in range(3)]
    base = random_rows(rng, 40)
    for step in range(4):
        items = []
        for b in range(B):
            n = 0 if (b == 2 and step % 2) else 30 + 7 * b + step
            d = np.stack([flip(base[i % 40], pick(rng, 3)) for i in range(max(n, 1))])
            v = (rng.random(max(n, 1)) < 0.8).astype(np.uint8) if b == 1 else None
            items.append(dict(n_query=n, graph_id=10 * step + b, desc=d, valid=v, xyz=None))
        for b, it in enumerate(items):  # query, then append
            got = bank.query(b, P, it["graph_id"], it["desc"][: it["n_query"]], None if it["valid"] is None else it["valid"])
            want = dbs[b].query(P, it["graph_id"], it["desc"][: it["n_query"]], it["valid"])
            assert_same(got, want, "step %d seq %d" % (step, b))
            assert got["index_query"] == want["index_query"] == len(dbs[b].maps)
            flat, node = bank.links(b, got, it["graph_id"], P["max_candidates"], base=3)
            assert [f - b * 6 for f in flat if f >= 0] == got["candidates"] and node == (it["graph_id"] - 3 if got["candidates"] else -1)
        st = bank.append(items)
        for b, it in enumerate(items):
            if it["n_query"]:
                dbs[b].add(it["graph_id"], it["desc"], it["valid"])
            assert st[b] == (pbr.OK if it["n_query"] else pbr.WARN_EMPTY_INPUT)
    # a re-queried stored id sees only its own sequence's index
    assert bank.query(0, P, 10, base)["index_query"] == 1 and bank.query(1, P, 10, base)["index_query"] == 4
    assert any(len(bank.query(b, P, 99, base)["candidates"]) > 0 for b in range(B))
