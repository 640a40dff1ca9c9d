"""The loop detector's CPU checker (tests/place_ref.py) against a direct pairwise loop, and on the reference's place-recognition and
loop-closing gtests with the exhaustive search standing in for HBST (no GPU needed)."""
import json
import os

import numpy as np
import pytest

import place_ref as pr
import point_align_ref as par
from oracle import binding as ob
from srrg2_proslam_amd import configs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def backend():
    import __graft_entry__ as g
    g.build()
    from test_ref_pins import OracleBackend
    return OracleBackend()


def near_copies(rng, base, n, flips):
    """rows of `base` with `flips` random bits flipped each"""
    out = base[rng.integers(0, len(base), n)].copy()
    for row in out:
        for b in rng.integers(0, 256, flips):
            row[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def assert_same_query(got, cands, corr, counts):
    assert got["candidates"] == cands
    assert list(got["counts"]) == list(counts)
    for a, b in zip(got["corr"], corr):
        assert np.array_equal(a, b)


def test_checker_against_pairwise_loop():
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    db = pr.Database()
    maps = [near_copies(rng, base, n, 20) for n in (17, 1, 33, 16)]
    for gid, d in enumerate(maps):
        valid = (rng.random(len(d)) < 0.8).astype(np.uint8) if gid == 2 else None
        db.add(10 + gid, d, valid)
    q = near_copies(rng, base, 30, 18)
    q[7] = q[3]  # a tie: the earlier query point wins
    qvalid = (rng.random(len(q)) < 0.85).astype(np.uint8)
    qvalid[3] = qvalid[7] = 1
    for thr, min_in, age, gid in ((40.0, 0, 0, 99), (45.5, 3, 1, 99), (60.0, 5, 0, 11), (256.0, 0, 2, 10), (0.0, -1, 0, 99)):
        P = pr.params(thr, age, min_in, max_candidates=8)
        got = db.query(P, gid, q, qvalid)
        assert_same_query(got, *pr.query_loop(db, P, gid, q, qvalid))
        for c in got["corr"]:
            assert (c["response"] < thr).all()


def test_tie_goes_to_the_earlier_query_point():
    rng = np.random.default_rng(1)
    ref = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    db = pr.Database()
    db.add(0, ref)
    q = np.repeat(ref, 3, axis=0)
    got = db.query(pr.params(1.0), 1, q)
    assert got["candidates"] == [0] and got["corr"][0]["fixed_idx"].tolist() == [0]
    got = db.query(pr.params(1.0), 1, q, np.array([0, 1, 1], np.uint8))
    assert got["corr"][0]["fixed_idx"].tolist() == [1]


def test_age_rule_wraps_for_a_requeried_older_map():
    rng = np.random.default_rng(2)
    d = rng.integers(0, 256, (20, 32), dtype=np.uint8)
    db = pr.Database()
    for gid in range(4):
        db.add(gid, d)
    P = pr.params(1.0, minimum_age_difference_to_candidates=1, relocalize_min_inliers=0)
    # re-query of graph id 1 (index 1): references 0 (age 1: fails), 1 (age 0: fails), 2 and 3 (older than... newer: wrap, pass)
    assert db.query(P, 1, d)["candidates"] == [2, 3]
    assert pr.query_loop(db, P, 1, d)[0] == [2, 3]
    # a new map (index 4): age 4 - r > 1 for r = 0, 1, 2
    assert db.query(P, 77, d)["candidates"] == [0, 1, 2]
    assert pr.age_ok(0, 5, 10**6) and not pr.age_ok(5, 5, 0) and pr.age_ok(6, 5, 0)


def test_empty_query_and_capacity():
    rng = np.random.default_rng(3)
    d = rng.integers(0, 256, (20, 32), dtype=np.uint8)
    db = pr.Database()
    for gid in range(5):
        db.add(gid, d)
    got = db.query(pr.params(1.0), 9, np.zeros((0, 32), np.uint8))
    assert got["status"] == pr.WARN_EMPTY_INPUT and got["candidates"] == []
    got = db.query(pr.params(1.0, max_candidates=3), 9, d)
    assert got["status"] == pr.ERR_CAPACITY and got["candidates"] == [0, 1, 2]
    assert db.query(pr.params(1.0), -1, d)["status"] == pr.ERR_RANGE


def test_feature_counts_of_the_2d_cases(backend):
    for which, n in pr.FEATURE_PINS.items():
        assert len(pr.features_2d(backend, which)) == n, which


def run_case(case, age=0):
    db = pr.Database()
    P = pr.params(case["thr"], age, case["min_inliers"])
    first = db.query(P, 0, case["ref"])
    assert first["candidates"] == []  # the first query finds nothing
    db.add(0, case["ref"])
    return db.query(P, 1, case["query"])


@pytest.mark.parametrize("dim", ["3d", "2d"])
def test_place_recognition_scenarios(backend, dim):
    cases = pr.recognition_3d(backend) if dim == "3d" else pr.recognition_2d(backend)[0]
    for case in cases:
        got = run_case(case)
        assert got["candidates"] == [0], case["name"]
        corr = got["corr"][0]
        assert (corr["response"] < case["thr"]).all(), case["name"]
        if case["perfect"]:
            assert len(corr) == case["pin"]
            assert (corr["fixed_idx"] == corr["moving_idx"]).all() and (corr["response"] == 0).all(), case["name"]
        else:
            assert len(corr) >= case["pin"], (case["name"], len(corr))  # exhaustive search only adds matches


def closure_runs(B):
    """the five test_loop_closing.cpp closures as database sequences -> [(scenario, query result, db)]"""
    sc = {s["name"]: s for s in par.scenarios(B)}
    out = []
    for name in ("kitti_00_00", "kitti_00_01"):
        s = sc[name]
        loop = configs.get("kitti")["loop"]
        db = pr.Database()
        db.add(0, s["moving_desc"], xyz=s["moving"])
        P = pr.params(s["max_distance"], 0, loop["relocalize_min_inliers"])
        out.append(([s], db.query(P, 1, s["fixed_desc"]), db, P, s))
    loop = configs.get("icl")["loop"]
    db = pr.Database()
    s01 = sc["icl_00_01"]
    db.add(0, s01["moving_desc"], xyz=s01["moving"])
    P = pr.params(s01["max_distance"], 0, loop["relocalize_min_inliers"])
    out.append(([s01], db.query(P, 1, s01["fixed_desc"]), db, P, s01))
    db2 = pr.Database()
    db2.add(0, s01["moving_desc"], xyz=s01["moving"])
    db2.add(1, s01["fixed_desc"], xyz=s01["fixed"])
    s50 = [sc["icl_00_50"], sc["icl_01_50"]]
    P = pr.params(s50[0]["max_distance"], 0, loop["relocalize_min_inliers"])
    out.append((s50, db2.query(P, 2, s50[0]["fixed_desc"]), db2, P, s50[0]))
    return out


def test_loop_closing_candidates_then_register(backend):
    for expect, got, db, P, q in closure_runs(backend):
        assert got["candidates"] == list(range(len(expect))), expect[0]["name"]
        for c, s in zip(got["candidates"], expect):
            m = db.maps[c]
            corr, _ = ob.bruteforce_match(q["fixed_desc"], m["desc"], s["max_distance"], 0.9)
            X, res, _ = par.align(par.from_loop_group(configs.get(s["config"])["loop"]), np.eye(4), q["fixed"], m["xyz"], corr)
            assert res["accepted"] == 1, s["name"]
            if s["truth"] is None:
                assert np.linalg.norm(par.pose_error(X, np.eye(4))) < 1e-5
            else:
                assert (np.abs(par.pose_error(X, s["truth"])) < np.asarray(s["bounds"])).all(), s["name"]


def test_unrelated_places_produce_no_candidate(backend):
    for s in par.unrelated(backend):
        db = pr.Database()
        db.add(0, s["moving_desc"])
        P = pr.params(s["max_distance"], 0, configs.get(s["config"])["loop"]["relocalize_min_inliers"])
        got = db.query(P, 1, s["fixed_desc"])
        assert got["candidates"] == [], (s["name"], got["counts"])


def test_detector_groups_match_the_shipped_configurations():
    with open(os.path.join(GOLDEN, "ref_conf_place.json")) as f:
        ref = json.load(f)
    for name in ("kitti", "euroc", "icl", "tum"):
        got, want = configs.get(name)["place"], ref[name]
        for k in ("maximum_descriptor_distance", "minimum_age_difference_to_candidates", "relocalize_min_inliers",
                  "maximum_leaf_size", "maximum_depth", "maximum_partitioning", "maximum_distance_for_merge"):
            assert got[k] == want[k], (name, k)
        assert want["maximum_distance_for_merge"] == 0  # the ambiguity filter is a no-op
    assert [configs.get(n)["place"]["minimum_age_difference_to_candidates"] for n in ("kitti", "icl", "euroc")] == [10, 1, 5]


def test_place_params_reads_the_detector():
    from srrg2_proslam_amd import formats
    text = '''"MultiLoopDetectorHBST3D" { "#id": 6, "maximum_descriptor_distance": 30, "maximum_depth": 12, "maximum_leaf_size": 50,
  "maximum_partitioning": 0.2, "maximum_distance_for_merge": 0, "minimum_age_difference_to_candidates": 7, "relocalize_min_inliers": 11 }
'''
    got = formats.place_params(formats.parse_conf(text))
    assert got == dict(maximum_descriptor_distance=30, maximum_depth=12, maximum_leaf_size=50, maximum_partitioning=0.2,
                       maximum_distance_for_merge=0, minimum_age_difference_to_candidates=7, relocalize_min_inliers=11)
