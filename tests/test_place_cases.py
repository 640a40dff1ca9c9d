"""The planted cases of tests/place_cases.py hold what their names say, on the CPU checker alone (no GPU needed): both forms of the
checker agree, the pairs below FLOOR bits are exactly the planted ones, every claim of a case is true of the checker's result, and
every structural position of POSITIONS is claimed by some case."""
import numpy as np
import pytest

import place_cases as pc
import place_ref as pr

CASES = pc.all_cases()
U64 = 1 << 64


class Env:
    """a case, the checker's database and results, and every matching pair with where it sits in the kernel's decomposition"""

    def __init__(self, case):
        self.case, self.db, self.P = case, pc.reference_db(case), case["P"]
        self.res = [self.db.query(self.P, q["gid"], q["desc"], q["valid"]) for q in case["queries"]]
        self.off, self.rows = pc.offsets(self.db)
        thr = np.float32(self.P["maximum_descriptor_distance"])
        self.lim = sum(1 for d in range(257) if np.float32(d) < thr)
        self.hits = pc.pairs_below(case, self.db, thr)
        self.near = pc.pairs_below(case, self.db, pc.FLOOR) if case["planted"] is not None else None

    def grow(self, m, point):
        return self.off[m] + int(np.flatnonzero(self.db.maps[m]["pidx"] == point)[0])

    def at_boundary(self, pred):
        """a pair at lim - 1 bits that `pred` accepts, whose query row also has a pair at exactly lim bits"""
        twins = {(b, q) for b, q, _, _, d in self.near if d == self.lim}
        return any(d == self.lim - 1 and (b, q) in twins and pred(b, q, m, p) for b, q, m, p, d in self.hits)

    def winner(self, b, m, point):
        c = self.res[b]["corr"][self.res[b]["candidates"].index(m)]
        return int(c["fixed_idx"][list(c["moving_idx"]).index(point)])


def slot_of(q, g):
    """(A tile, accumulator register, lane) of query row q against global database row g"""
    return ((q % 64) // 16, q % 4, 16 * ((q % 16) // 4) + g % 16)


def check_slots(e, what, v):
    valid = e.case["queries"][0]["valid"]
    assert (valid is not None) == (what == "all_valid")
    live = [q for q in range(64) if valid is None or valid[q]]
    want = {slot_of(q, p) for q in live for p in range(16)}
    assert len(want) == 16 * len(live) and (valid is None or len(live) == 42)
    for d, pairs in ((e.lim - 1, e.hits), (e.lim, e.near)):
        got = {slot_of(q, e.grow(m, p)) for _, q, m, p, dd in pairs if dd == d}
        assert got == want, d
    assert {q // 64 for _, q, _, _, _ in e.hits} == {v["wave"]}
    assert all(valid is None or valid[q] for _, q, _, _, _ in e.hits)


def check_row(e, what, v):
    if what.isdigit():
        assert v == int(what) and e.at_boundary(lambda b, q, m, p: e.grow(m, p) == v)
    elif what == "last_before_pads":
        m = max(i for i, o in enumerate(e.off) if o <= v)
        n = len(e.db.maps[m]["desc"])
        assert v == e.off[m] + n - 1 and n % 16 != 0 and e.at_boundary(lambda b, q, mm, p: e.grow(mm, p) == v)
    elif what == "one_row_map":
        assert len(e.db.maps[v]["desc"]) == 1 and e.at_boundary(lambda b, q, m, p: m == v)
    elif what == "straddles_slice":
        sl = {e.grow(m, p) // 1024 for _, _, m, p, _ in e.hits if m == v}
        assert len(sl) == 2
    elif what == "four_maps_in_chunk":
        assert [len(e.db.maps[m]["desc"]) for m in v] == [16] * 4 and [e.off[m] - e.off[v[0]] for m in v] == [0, 16, 32, 48]
        assert e.off[v[0]] % 64 == 0
        counts = [int(e.res[0]["counts"][m]) for m in v]
        assert len(set(counts)) == 4 and 0 in counts  # a count credited to the neighbouring map shows
    else:
        raise KeyError(what)


def check_query(e, what, v):
    n = len(e.case["queries"][0]["desc"])
    if what == "last_odd":
        assert v == n - 1 and n % 16 != 0
    else:
        assert v == int(what)
    assert e.at_boundary(lambda b, q, m, p: q == v)


def check_thr(e, what, v):
    assert "%g" % e.P["maximum_descriptor_distance"] == what and e.lim == v["lim"]
    q0 = e.case["queries"][0]["desc"][:1]
    d = np.concatenate([pr.distances(q0, m["desc"])[0] for m in e.db.maps[:2]])
    assert sorted(d[:6]) == list(pc.SPECIAL) and d[6] > 64
    assert all(len(m["desc"]) % 16 != 0 for m in e.db.maps)  # pad rows behind every map
    got = sorted(dd for b, q, m, p, dd in e.hits if (b, q) == (0, 0) and m < 2 and (m, p) != (1, 3))
    assert got == [x for x in pc.SPECIAL if x < e.lim] and len(got) == v["special"]
    stored = sum(len(m["desc"]) for m in e.db.maps)
    if e.lim == 257:
        assert len(e.hits) == 4 * stored  # every Valid query row against every stored row, and no pad row
        c = e.res[1]["corr"][0]  # the all-one row alone against the all-zero row: 256 bits is the best there is
        assert (c["moving_idx"][0], c["response"][0]) == (0, 256.0)
    if e.lim == 0:
        assert not e.hits and e.res[0]["candidates"] == []


def check_tie(e, what, v):
    for t in v if isinstance(v, list) else [v]:
        (m, p), qs, b = t["row"], t["qs"], 0
        d = {q: dd for bb, q, mm, pp, dd in e.hits if (bb, mm, pp) == (b, m, p)}
        assert sorted(d) == sorted(qs) and e.winner(b, m, p) == t["winner"]
        if what == "closer_later":
            assert d[qs[0]] == d[qs[1]] == d[qs[2]] + 1 and qs[2] > max(qs[:2]) and t["winner"] == qs[2]
            continue
        assert d[qs[0]] == d[qs[1]] and t["winner"] == min(qs)
        a, c = qs
        assert {"same_tile": a // 16 == c // 16 and a % 4 != c % 4, "waves": a // 64 != c // 64 and a // 256 == c // 256,
                "qblocks": a // 256 != c // 256}[what]


def check_count(e, what, v):
    b, m = v["b"], v["map"]
    mi = e.P["relocalize_min_inliers"]
    assert int(e.res[b]["counts"][m]) == {"m": mi, "m+1": mi + 1, "0": 0}[what] and mi > 1
    assert (m in e.res[b]["candidates"]) == (what == "m+1")
    assert pr.age_ok(e.res[b]["index_query"], m, e.P["minimum_age_difference_to_candidates"])  # the inlier rule alone decides
    if what != "0":
        per_row = {}
        for bb, q, mm, p, _ in e.hits:
            if (bb, mm) == (b, m):
                per_row[p] = per_row.get(p, 0) + 1
        assert max(per_row.values()) > 1  # several query rows on one stored row


def check_age(e, what, v):
    b, m = v["b"], v["map"]
    diff = (e.res[b]["index_query"] - m) % U64
    ma = e.P["minimum_age_difference_to_candidates"]
    assert {"eq": diff == ma, "+1": diff == ma + 1, "wrap": diff > 1 << 63}[what]
    assert (m in e.res[b]["candidates"]) == (what != "eq")
    assert pr.inliers_ok(e.res[b]["counts"][m], e.P["relocalize_min_inliers"])  # the age rule alone decides


def check_strides(e, what, v):
    assert what == "batch3" and len(e.case["queries"]) == 3
    assert len({tuple(r["candidates"]) for r in e.res}) == 3 and len({tuple(r["counts"]) for r in e.res}) == 3


def check_gather(e, what, v):
    kind, _, arg = what.rpartition("_")
    if kind == "valid":
        valid = e.case["queries"][v]["valid"]
        assert valid is not None and int(valid.sum()) == int(arg) and len(valid) == 130
        if int(arg) in (63, 64, 65):
            assert valid[63] and valid[64] and not valid[0] and not valid[-1]  # one run across the 64-row rounds
        assert bool(e.res[v]["candidates"]) == (int(arg) > 0)
    elif kind == "map_rows":
        assert len(e.db.maps[v]["desc"]) == int(arg) and any(v in r["candidates"] for r in e.res)
    elif what == "masked_map":
        valid = e.case["maps"][v]["valid"]
        assert valid is not None and 0 < valid.sum() < len(valid) and not valid[0] and any(v in r["candidates"] for r in e.res)
    elif what == "overflow":
        assert e.res[v]["status"] == pr.ERR_CAPACITY and len(e.res[v]["candidates"]) == e.P["max_candidates"]
    elif what == "empty_query":
        assert e.res[v]["status"] == pr.WARN_EMPTY_INPUT and not len(e.case["queries"][v]["desc"])
    elif what == "negative_gid":
        assert e.res[v]["status"] == pr.ERR_RANGE and len(e.case["queries"][v]["desc"])
    elif kind == "slots":
        assert len(e.case["queries"]) * e.P["max_candidates"] == int(arg)
    else:
        raise KeyError(what)


def check_plain(key):
    def check(e, what, v):
        got = [r[key] for r in e.res]
        assert [list(map(int, g)) if key != "index_query" else int(g) for g in got] == v, (got, v)
    return check


def check_winners(e, what, v):
    for (b, m, p), q in v.items():
        assert e.winner(b, m, p) == q


CHECKS = dict(slots=check_slots, row=check_row, query=check_query, thr=check_thr, tie=check_tie, count=check_count, age=check_age,
              strides=check_strides, gather=check_gather, counts=check_plain("counts"), candidates=check_plain("candidates"),
              index_query=check_plain("index_query"), winners=check_winners)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_holds_what_it_claims(case):
    e = Env(case)
    for q, want in zip(case["queries"], e.res):
        if want["status"] == pr.ERR_RANGE:
            assert want["candidates"] == []
            continue
        cands, corr, counts = pr.query_loop(e.db, e.P, q["gid"], q["desc"], q["valid"])
        assert want["candidates"] == cands and list(want["counts"]) == list(counts)
        assert len(want["corr"]) == len(corr) and all(np.array_equal(a, b) for a, b in zip(want["corr"], corr))
    if case["planted"] is not None:
        assert e.P["maximum_descriptor_distance"] <= 64
        assert e.near == case["planted"]  # nothing but the planted pairs below FLOOR, at the planted distances
        assert e.hits == [p for p in case["planted"] if p[4] < e.lim]
    else:
        assert e.rows <= 200
    for claim, v in case["claims"].items():
        kind, _, what = claim.partition(":")
        CHECKS[kind](e, what, v)


def test_sizes_stay_small():
    for case in CASES:
        _, rows = pc.offsets(pc.reference_db(case))
        nq = max(len(q["desc"]) for q in case["queries"])
        assert rows <= 3100 and (nq <= 600 or (nq == 65536 and rows <= 64)), case["name"]


def test_every_position_is_claimed():
    claimed = {k for c in CASES for k in c["claims"]}
    missing = [p for p in pc.POSITIONS if p not in claimed]
    assert not missing, missing
    assert all(k.partition(":")[0] in CHECKS for k in claimed)


def test_gather_pairs_reference():
    case = pc.by_name("gather_overflow")
    db = pc.reference_db(case)
    for b, q in enumerate(case["queries"]):
        res = db.query(case["P"], q["gid"], q["desc"], q["valid"])
        slots = pr.gather_pairs(db, res, q["desc"], q["xyz"], q["valid"], case["P"]["max_candidates"])
        assert len(slots) == 2 and all(np.array_equal(s["X"], np.eye(4, dtype=np.float32)) for s in slots)
        if b in (1, 2):
            assert [(s["n_fixed"], s["n_moving"]) for s in slots] == [(0, 0)] * 2
            continue
        keep = np.arange(len(q["desc"])) if q["valid"] is None else np.flatnonzero(q["valid"])
        for k, s in enumerate(slots):
            assert (s["n_fixed"], s["n_moving"]) == (len(keep), len(db.maps[k]["desc"]))  # over max_candidates: the first two stay
            assert np.array_equal(s["fixed_desc"], q["desc"][keep]) and np.array_equal(s["fixed_xyz"], q["xyz"][keep])
            assert np.array_equal(s["moving_desc"], db.maps[k]["desc"]) and np.array_equal(s["moving_xyz"], db.maps[k]["xyz"])
