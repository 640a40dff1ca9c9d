"""Inputs of exactly known content for the loop detector's tests, and the helpers its GPU tests share.

Independent random 256-bit rows are 128 +- 8 bits apart, so a database and a query of random rows hold no pair at any threshold of at
most 64 bits (8 sigma).  A case PLANTS its pairs: a group is one random base row; each of its database rows (map, point) and query
rows (query, index) is the base with a chosen set of bits flipped, so the distance of two rows of a group is the size of the symmetric
difference of their bit sets.  `planted` lists every pair of a group closer than FLOOR bits as (query, index, map, point, distance):
a pair one bit under the threshold, its twin exactly on it, ties, counted pairs.  tests/test_place_cases.py checks on the CPU
checker alone that these are ALL the pairs below FLOOR, at these distances, so the matched set of a case is its planted set below
the threshold and nothing else.  Dense cases (planted None: all-zero and all-one descriptors, thresholds up to infinity, at most 200
rows) match nearly everything; their expectation is the checker's.

A case: dict(name, maps [dict(gid, desc, xyz, valid)], queries [dict(gid, desc, xyz, valid)], P (place_ref.params), planted, claims).
`claims` maps a position of POSITIONS (or a further "kind:what" name) to its detail; test_place_cases.py verifies each on the checker
(CHECKS there) and that every position of POSITIONS is claimed by some case.  Point indices count the rows as uploaded (before a
`valid` mask); the global row of a stored row is its map's offset (maps padded to 16 rows) plus its rank among the map's Valid rows.
"""
import functools

import numpy as np

import place_ref as pr

FLOOR = 80          # every pair of a sparse case below this many bits is a planted one
LIM = 33            # the threshold of the sparse cases: a pair at 32 bits matches, its twin at 33 does not
SPECIAL = (0, 1, 32, 33, 255, 256)
THRESHOLDS = (-1.0, 0.0, 0.5, 1.0, 32.5, 33.0, 255.0, 256.0, 256.5, 300.0, float("inf"))

POSITIONS = (
    ["slots:all", "slots:all_valid"]
    + ["row:%d" % g for g in (0, 15, 16, 63, 64, 1023, 1024)]
    + ["row:last_before_pads", "row:one_row_map", "row:straddles_slice", "row:four_maps_in_chunk"]
    + ["query:%d" % q for q in (0, 15, 16, 63, 64, 255, 256, 65535)] + ["query:last_odd"]
    + ["thr:%g" % t for t in THRESHOLDS]
    + ["tie:same_tile", "tie:waves", "tie:qblocks", "tie:closer_later"]
    + ["count:m", "count:m+1", "count:0", "age:eq", "age:+1", "age:wrap"]
    + ["strides:batch3"]
    + ["gather:valid_%d" % k for k in (0, 1, 63, 64, 65, 130)]
    + ["gather:map_rows_%d" % n for n in (1, 16, 17)]
    + ["gather:masked_map", "gather:overflow", "gather:empty_query", "gather:negative_gid"]
    + ["gather:slots_%d" % n for n in (1, 3, 4, 5)]
)


# ---------------------------------------------------------------------------------------------------------------- generators
def random_rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip(row, bits):
    out = np.array(row, dtype=np.uint8, copy=True)
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def pick(rng, n, exclude=()):
    """n distinct bit positions outside `exclude`"""
    free = np.setdiff1d(np.arange(256), np.asarray(list(exclude), np.int64))
    return tuple(int(b) for b in rng.permutation(free)[:n])


def ones_row(k):
    """a descriptor with its first k bits set"""
    return np.packbits(np.arange(256) < k)


def _spec(s):
    s = dict(n=s) if isinstance(s, int) else dict(s)
    s.setdefault("valid", None)
    return s


def _live(item, i):
    """is row i of a map or a query Valid"""
    return item["valid"] is None or item["valid"][i] != 0


def assemble(name, rng, maps, queries, groups, P, claims, floor=FLOOR):
    """maps / queries: a row count or dict(n, gid, valid) each (gid defaults to the map index / 1000 + the query index);
    groups: dict(rows={(map, point): bits}, queries={(query, index): bits})"""
    ms, qs = [], []
    for i, s in enumerate(map(_spec, maps)):
        ms.append(dict(gid=s.get("gid", i), desc=random_rows(rng, s["n"]), valid=s["valid"],
                       xyz=rng.integers(-50, 50, (s["n"], 3)).astype(np.float32)))
    for i, s in enumerate(map(_spec, queries)):
        qs.append(dict(gid=s.get("gid", 1000 + i), desc=random_rows(rng, s["n"]), valid=s["valid"],
                       xyz=rng.integers(-50, 50, (s["n"], 3)).astype(np.float32)))
    planted, seen_r, seen_q = [], set(), set()
    for g in groups:
        base = random_rows(rng, 1)[0]
        for (m, p), bits in g["rows"].items():
            assert (m, p) not in seen_r and 0 <= p < len(ms[m]["desc"]), (name, m, p)
            seen_r.add((m, p))
            ms[m]["desc"][p] = flip(base, bits)
        for (b, q), bits in g["queries"].items():
            assert (b, q) not in seen_q and 0 <= q < len(qs[b]["desc"]), (name, b, q)
            seen_q.add((b, q))
            qs[b]["desc"][q] = flip(base, bits)
        for (b, q), bq in g["queries"].items():
            for (m, p), br in g["rows"].items():
                d = len(set(bq) ^ set(br))
                if d < floor and _live(qs[b], q) and _live(ms[m], p):
                    planted.append((b, q, m, p, d))
    return dict(name=name, maps=ms, queries=qs, P=P, planted=sorted(planted), claims=claims)


def boundary_group(rng, b, q, hit, twin, d=LIM - 1):
    """query row (b, q) with database row `hit` at d bits and database row `twin` at d + 1"""
    bh = pick(rng, d)
    return dict(rows={hit: bh, twin: pick(rng, d + 1, exclude=bh)}, queries={(b, q): ()})


def case_slots(with_valid):
    """the 64 query rows of one wave x the 16 positions of a tile: map 0 holds a row at 32 bits for each of the 1024 (t, r, lane),
    map 1 its twin at 33 bits at the same tile position; map 2 is one all-zero row"""
    rng = np.random.default_rng(101 + with_valid)
    n = 70
    valid = (np.arange(n) % 3 != 0).astype(np.uint8) if with_valid else None
    groups = []
    for q in range(64):
        rows = {}
        for p in range(16):
            bh = pick(rng, LIM - 1)
            rows[(0, 16 * q + p)] = bh
            rows[(1, 16 * q + p)] = pick(rng, LIM, exclude=bh)
        groups.append(dict(rows=rows, queries={(0, q): ()}))
    live = 64 if valid is None else int(valid[:64].sum())
    claims = {"slots:all_valid" if with_valid else "slots:all": dict(wave=0), "counts": [[16 * live, 0, 0]], "candidates": [[0]]}
    c = assemble("slots_valid" if with_valid else "slots", rng, [1024, 1024, 1], [dict(n=n, valid=valid)], groups,
                 pr.params(float(LIM), 0, 0), claims)
    # a query row that is absent or not Valid enters the kernel as zeros: only an all-zero stored row would show one that counted
    c["maps"][2]["desc"][0] = 0
    return c


def case_rows():
    """map 0: 1030 rows (global 0 .. 1029, pads to 1040, across the slice boundary); map 1: one row (1040); map 2: 32 rows (1056);
    maps 3 .. 6: 16 rows each, the chunk 1088 .. 1151, with 1, 2, 0 and 3 matches"""
    rng = np.random.default_rng(102)
    sizes = [1030, 1, 32, 16, 16, 16, 16]
    spots = [0, 15, 16, 63, 64, 1023, 1024, 1029]
    groups = [boundary_group(rng, 0, i, (0, g), (0, 200 + 16 * i + i)) for i, g in enumerate(spots)]
    groups.append(boundary_group(rng, 0, 8, (1, 0), (2, 31)))
    groups.append(boundary_group(rng, 0, 9, (3, 15), (4, 0)))
    groups.append(dict(rows={(4, 7): ()}, queries={(0, 10): pick(rng, 5), (0, 11): pick(rng, LIM - 1)}))
    groups.append(dict(rows={(6, 0): (), (6, 15): pick(rng, 3), (5, 3): pick(rng, 70)}, queries={(0, 12): pick(rng, 4)}))
    groups.append(dict(rows={(6, 8): ()}, queries={(0, 13): ()}))
    claims = {"row:%d" % g: g for g in spots[:7]}
    claims.update({"row:last_before_pads": 1029, "row:one_row_map": 1, "row:straddles_slice": 0, "row:four_maps_in_chunk": [3, 4, 5, 6],
                   "counts": [[8, 1, 0, 1, 2, 0, 3]], "candidates": [[0, 1, 3, 4, 6]]})
    return assemble("rows", rng, sizes, [20], groups, pr.params(float(LIM), 0, 0, max_candidates=8), claims)


def case_queries():
    rng = np.random.default_rng(103)
    spots = [0, 15, 16, 63, 64, 255, 256, 260]
    groups = [boundary_group(rng, 0, q, (i % 2, 2 * i), (1 - i % 2, 2 * i + 1)) for i, q in enumerate(spots)]
    claims = {"query:%d" % q: q for q in spots[:7]}
    claims.update({"query:last_odd": 260, "counts": [[4, 4]], "candidates": [[0, 1]]})
    return assemble("queries", rng, [20, 30], [261], groups, pr.params(float(LIM), 0, 0), claims)


def case_query_65535():
    """65536 query rows of which a mask keeps five (the pairwise loop of the CPU test skips the others); the GPU test also runs it
    without the mask"""
    rng = np.random.default_rng(104)
    valid = np.zeros(65536, np.uint8)
    valid[[0, 1000, 65533, 65534, 65535]] = 1
    groups = [boundary_group(rng, 0, 65535, (0, 3), (0, 5)),
              dict(rows={(0, 20): ()}, queries={(0, 65534): pick(rng, 9), (0, 65533): pick(rng, 9), (0, 0): pick(rng, 30)})]
    claims = {"query:65535": 65535, "counts": [[4]], "candidates": [[0]], "winners": {(0, 0, 20): 65533}}
    return assemble("query_65535", rng, [40], [dict(n=65536, valid=valid)], groups, pr.params(float(LIM), 0, 0), claims)


def case_threshold(thr):
    """distances 0, 1, 32, 33, 255 and 256 from an all-zero and an all-one query row, in maps of 3, 4 and 17 rows (13, 12, 15 pads);
    the second query is the all-one row alone, so that 256 bits is the best distance of the all-zero stored row"""
    rng = np.random.default_rng(105)
    c = assemble("thr_%g" % thr, rng, [3, 4, 17], [3, 1], [], pr.params(thr, 0, 0), {}, floor=0)
    c["maps"][0]["desc"][:] = [ones_row(0), ones_row(1), ones_row(32)]
    c["maps"][1]["desc"][:3] = [ones_row(33), ones_row(255), ones_row(256)]
    c["queries"][0]["desc"][:2] = [ones_row(0), ones_row(256)]
    c["queries"][1]["desc"][0] = ones_row(256)
    c["planted"] = None
    lim = sum(1 for d in range(257) if np.float32(d) < np.float32(thr))
    c["claims"] = {"thr:%g" % thr: dict(lim=lim, special=sum(1 for d in SPECIAL if d < lim))}
    return c


def case_ties():
    rng = np.random.default_rng(106)

    def tie(point, a, b, later=None):
        common = pick(rng, 10)
        qs = {(0, a): common + pick(rng, 10, exclude=common), (0, b): common + pick(rng, 10, exclude=common)}
        if later is not None:
            qs[(0, later)] = pick(rng, 19)
        return dict(rows={(0, point): ()}, queries=qs)

    groups = [tie(2, 3, 9), tie(3, 5, 11, 13), tie(4, 20, 150), tie(5, 21, 151, 200), tie(6, 10, 300), tie(7, 12, 301, 310)]
    claims = {"tie:same_tile": dict(row=(0, 2), qs=[3, 9], winner=3), "tie:waves": dict(row=(0, 4), qs=[20, 150], winner=20),
              "tie:qblocks": dict(row=(0, 6), qs=[10, 300], winner=10),
              "tie:closer_later": [dict(row=(0, 3), qs=[5, 11, 13], winner=13), dict(row=(0, 5), qs=[21, 151, 200], winner=200),
                                   dict(row=(0, 7), qs=[12, 301, 310], winner=310)],
              "counts": [[15]], "candidates": [[0]]}
    return assemble("ties", rng, [40], [320], groups, pr.params(float(LIM), 0, 0), claims)


def case_counts():
    """m = 5: map 0 gets 5 matches (3 + 2 query rows on two rows), map 1 gets 6 (4 + 2), map 2 none"""
    rng = np.random.default_rng(107)
    groups = [dict(rows={(0, 1): ()}, queries={(0, q): pick(rng, 3 + q % 7) for q in (0, 1, 2)}),
              dict(rows={(0, 17): ()}, queries={(0, q): pick(rng, 3 + q % 7) for q in (3, 4)}),
              dict(rows={(1, 0): ()}, queries={(0, q): pick(rng, 3 + q % 7) for q in (5, 6, 7, 8)}),
              dict(rows={(1, 20): ()}, queries={(0, q): pick(rng, 3 + q % 7) for q in (70, 71)})]
    claims = {"count:m": dict(b=0, map=0), "count:m+1": dict(b=0, map=1), "count:0": dict(b=0, map=2), "counts": [[5, 6, 0]],
              "candidates": [[1]]}
    return assemble("counts", rng, [18, 21, 16], [72], groups, pr.params(float(LIM), 0, 5), claims)


def case_age():
    """five maps with two matches each, minimum age 2, the query re-queries map 3: differences 3, 2, 1, 0 and -1 (wraps)"""
    rng = np.random.default_rng(108)
    groups = [dict(rows={(m, 2 + m): ()}, queries={(0, 2 * m): pick(rng, 6), (0, 2 * m + 1): pick(rng, 7)}) for m in range(5)]
    maps = [dict(n=10 + m, gid=50 + m) for m in range(5)]
    claims = {"age:+1": dict(b=0, map=0), "age:eq": dict(b=0, map=1), "age:wrap": dict(b=0, map=4), "index_query": [3],
              "counts": [[2] * 5], "candidates": [[0, 4]]}
    return assemble("age", rng, maps, [dict(n=12, gid=53)], groups, pr.params(float(LIM), 2, 1), claims)


def case_strides():
    """three queries with different planted pairs against four maps"""
    rng = np.random.default_rng(109)
    groups = [dict(rows={(0, 3): ()}, queries={(0, 1): pick(rng, 4), (0, 30): pick(rng, 9)}),
              dict(rows={(2, 16): ()}, queries={(0, 5): pick(rng, 2)}),
              dict(rows={(1, 0): (), (1, 39): pick(rng, 8)}, queries={(1, 44): pick(rng, 5), (1, 2): pick(rng, 5)}),
              dict(rows={(3, 4): ()}, queries={(2, 0): pick(rng, 12), (2, 19): pick(rng, 12), (2, 20): pick(rng, 11)}),
              dict(rows={(0, 30): ()}, queries={(2, 7): ()})]
    claims = {"strides:batch3": True, "counts": [[2, 0, 1, 0], [0, 4, 0, 0], [1, 0, 0, 3]], "candidates": [[0, 2], [1], [0, 3]]}
    return assemble("strides", rng, [33, 40, 17, 5], [31, 45, 21], groups, pr.params(float(LIM), 0, 0, max_candidates=3), claims)


def _run(n, first, count):
    v = np.zeros(n, np.uint8)
    v[first: first + count] = 1
    return v


def _middle_valid(spec):
    """the index of the middle Valid row of a map or query spec, None where it has none"""
    keep = np.arange(spec["n"]) if spec["valid"] is None else np.flatnonzero(spec["valid"])
    return int(keep[len(keep) // 2]) if len(keep) else None


def gather_case(name, seed, maps, queries, max_candidates, claims, skip_maps=()):
    """one group over the whole case: the middle Valid row of every query and the middle Valid row of every map (but `skip_maps`)
    are within 10 bits of each other, so every such map is a candidate of every query that has a Valid row"""
    rng = np.random.default_rng(seed)
    g = dict(rows={}, queries={})
    for m, s in enumerate(map(_spec, maps)):
        if _middle_valid(s) is not None and m not in skip_maps:
            g["rows"][(m, _middle_valid(s))] = pick(rng, 5)
    for b, s in enumerate(map(_spec, queries)):
        if s["n"] and s.get("gid", 0) >= 0 and _middle_valid(s) is not None:
            g["queries"][(b, _middle_valid(s))] = pick(rng, 5)
    claims = dict(claims)
    claims["gather:slots_%d" % (len(queries) * max_candidates)] = True
    return assemble(name, rng, maps, queries, [g], pr.params(float(LIM), 0, 0, max_candidates=max_candidates), claims)


def gather_cases():
    masked = (np.arange(40) % 5 != 1).astype(np.uint8)
    masked[:3] = 0
    maps = [1, 16, 17, dict(n=40, valid=masked)]
    runs = {0: _run(130, 0, 0), 1: _run(130, 64, 1), 63: _run(130, 40, 63), 64: _run(130, 33, 64), 65: _run(130, 31, 65), 130: _run(130, 0, 130)}
    holes = _run(130, 10, 110)
    holes[[20, 63, 100]] = 0
    queries = [dict(n=130, valid=v) for v in runs.values()] + [dict(n=130, valid=holes), dict(n=97)]
    claims = {"gather:valid_%d" % k: b for b, k in enumerate(runs)}
    claims.update({"gather:map_rows_1": 0, "gather:map_rows_16": 1, "gather:map_rows_17": 2, "gather:masked_map": 3,
                   "candidates": [[]] + [[0, 1, 2, 3]] * 7})
    out = [gather_case("gather_valid", 201, maps, queries, 4, claims)]
    out.append(gather_case("gather_overflow", 202, maps, [dict(n=50), dict(n=0), dict(n=50, gid=-7), dict(n=20, valid=_run(20, 3, 9))], 2,
                           {"gather:overflow": 0, "gather:empty_query": 1, "gather:negative_gid": 2, "candidates": [[0, 1], [], [], [0, 1]]}))
    out.append(gather_case("gather_slots_1", 203, [17], [dict(n=9, valid=_run(9, 2, 4))], 1, {"candidates": [[0]]}))
    out.append(gather_case("gather_slots_3", 204, [5, 16, 3], [dict(n=66, valid=_run(66, 60, 6))], 3, {"candidates": [[0, 1]]}, skip_maps=(2,)))
    out.append(gather_case("gather_slots_4", 206, [16, 33], [dict(n=64, valid=_run(64, 1, 63)), 65], 2, {"candidates": [[0, 1], [0, 1]]}))
    out.append(gather_case("gather_slots_5", 205, [20], [7, 0, 70, dict(n=70, valid=_run(70, 0, 0)), 65], 1,
                           {"candidates": [[0], [], [0], [], [0]]}))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    """every case, generated once (shared by the tests: read only)"""
    out = [case_slots(False), case_slots(True), case_rows(), case_queries(), case_query_65535()]
    out += [case_threshold(t) for t in THRESHOLDS]
    out += [case_ties(), case_counts(), case_age(), case_strides()] + gather_cases()
    return out


def by_name(name):
    return {c["name"]: c for c in all_cases()}[name]


# ------------------------------------------------------------------------------------------------------- the checker's side
def reference_db(case):
    db = pr.Database()
    for m in case["maps"]:
        db.add(m["gid"], m["desc"], m["valid"], m["xyz"])
    return db


def offsets(db):
    """the global row of every map's first stored row (maps padded to 16 rows), and the padded total"""
    off, rows = [], 0
    for m in db.maps:
        off.append(rows)
        rows += (len(m["desc"]) + 15) // 16 * 16
    return off, rows


def pairs_below(case, db, bound):
    """every (query, index, map, point, distance) of a Valid query row and a stored row with (float) distance < bound"""
    out = []
    for b, q in enumerate(case["queries"]):
        if q["gid"] < 0 or not len(q["desc"]):
            continue
        qv = np.arange(len(q["desc"])) if q["valid"] is None else np.flatnonzero(q["valid"])
        for mi, m in enumerate(db.maps):
            d = pr.distances(q["desc"][qv], m["desc"])
            for i, r in zip(*np.nonzero(d.astype(np.float32) < np.float32(bound))):
                out.append((b, int(qv[i]), mi, int(m["pidx"][r]), int(d[i, r])))
    return sorted(out)


# ------------------------------------------------------------------------------------------------- shared by the GPU tests
class Pair:
    """the device database and the checker's, kept in step"""

    def __init__(self, ctx, ops):
        self.dev, self.ref = ops.PlaceDatabase(ctx), pr.Database()

    def add(self, gid, desc, xyz=None, valid=None):
        self.dev.add(gid, desc, xyz, valid)
        self.ref.add(gid, desc, valid, xyz)


def cparams(p):
    return pr.params(p.maximum_descriptor_distance, p.minimum_age_difference_to_candidates, p.relocalize_min_inliers, p.max_candidates)


def assert_same(got, want, what=""):
    assert got["status"] == want["status"], (what, got["status"], want["status"])
    assert got["candidates"] == want["candidates"], (what, got["candidates"], want["candidates"])
    if want["status"] >= 0 and want["status"] != pr.WARN_EMPTY_INPUT:
        assert np.array_equal(np.asarray(got["counts"], np.int64), want["counts"]), what
    assert len(got["corr"]) == len(want["corr"]), what
    for a, b in zip(got["corr"], want["corr"]):
        assert len(a) == len(b), (what, len(a), len(b))
        for k in ("fixed_idx", "moving_idx"):
            assert np.array_equal(a[k], b[k]), (what, k)
        assert np.array_equal(a["response"].astype(np.float32).view(np.uint32), b["response"].astype(np.float32).view(np.uint32)), what


def batch_query(ctx, ops, pair, P, items, query_stride=None, with_valid=False, corr_stride=None):
    """items: (graph_id, desc[, valid]) -> per-query result dicts of the batch entry"""
    qs = query_stride or max(max(len(i[1]) for i in items), 1)
    q = ops.PlaceQueries(0, len(items), qs, P.max_candidates, pair.dev, with_valid=with_valid, corr_stride=corr_stride)
    for b, it in enumerate(items):
        q.upload(b, it[0], it[1], None, it[2] if len(it) > 2 else None)
    ops.place_query_batch(ctx, pair.dev, P, q)
    ctx.synchronize()
    return [q.result_of(b, pair.dev.size()[0]) for b in range(len(items))]


def both_entries(ctx, ops, pair, P, gid, desc, valid=None, what=""):
    want = pair.ref.query(cparams(P), gid, desc, valid)
    got_b = batch_query(ctx, ops, pair, P, [(gid, desc, valid)], with_valid=valid is not None)[0]
    assert_same(got_b, want, what + " batch")
    if want["status"] >= 0:
        assert_same(pair.dev.query(P, gid, desc, valid), want, what + " host")
    return want
