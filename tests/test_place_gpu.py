"""The loop detector's candidate search on the device (prs_place_query_batch / prs_place_query / the C++ adapter) equals the CPU
checker (tests/place_ref.py) bit for bit -- match counts, candidate lists, correspondences, status -- and the chained detector
(ops.LoopDetectorBatch: search, gather, brute-force matcher, loop aligner) accepts the five closures of test_loop_closing.cpp."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import place_ref as pr
import point_align_ref as par
from place_cases import Pair, assert_same, batch_query, both_entries, cparams
from srrg2_proslam_amd import _lib, configs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import ops
    from test_ref_pins import OracleBackend
    assert torch.cuda.is_available()
    ctx = ops.Context(0)
    yield ctx, ops, OracleBackend()
    ctx.close()


def near(rng, base, n, flips):
    out = base[rng.integers(0, len(base), n)].copy()
    bits = rng.integers(0, 256, (n, flips))
    for i in range(n):
        for b in bits[i]:
            out[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def test_reference_scenarios(env):
    ctx, ops, B = env
    cases = pr.recognition_3d(B) + pr.recognition_2d(B)[0]
    for case in cases:
        pair = Pair(ctx, ops)
        P = ops.place_params(dict(maximum_descriptor_distance=case["thr"], minimum_age_difference_to_candidates=0,
                                  relocalize_min_inliers=case["min_inliers"]))
        first = both_entries(ctx, ops, pair, P, 0, case["ref"], what=case["name"] + " first")
        assert first["candidates"] == []
        pair.add(0, case["ref"])
        want = both_entries(ctx, ops, pair, P, 1, case["query"], what=case["name"])
        assert want["candidates"] == [0]
        corr = want["corr"][0]
        if case["perfect"]:
            assert len(corr) == case["pin"] and (corr["fixed_idx"] == corr["moving_idx"]).all() and (corr["response"] == 0).all()
        else:
            assert len(corr) >= case["pin"]


def test_empty_and_one_map_database(env):
    ctx, ops, _ = env
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (50, 32), dtype=np.uint8)
    pair = Pair(ctx, ops)
    P = ops.place_params(dict(maximum_descriptor_distance=40.0, minimum_age_difference_to_candidates=0, relocalize_min_inliers=0))
    assert both_entries(ctx, ops, pair, P, 3, near(rng, base, 20, 10), what="empty db")["candidates"] == []
    pair.add(0, base)
    assert both_entries(ctx, ops, pair, P, 3, near(rng, base, 20, 10), what="one map")["candidates"] == [0]


@pytest.mark.parametrize("thr", [0.0, 1.0, 256.0, 33.0])
def test_tile_padding_edges(env, thr):
    ctx, ops, _ = env
    rng = np.random.default_rng(int(thr) + 7)
    base = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    pair = Pair(ctx, ops)
    sizes = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 1040]
    for gid, n in enumerate(sizes):
        valid = (rng.random(n) < 0.9).astype(np.uint8) if gid % 3 == 2 else None
        pair.add(gid, near(rng, base, n, 6), valid=valid)
    P = ops.place_params(dict(maximum_descriptor_distance=thr, minimum_age_difference_to_candidates=0, relocalize_min_inliers=0),
                         max_candidates=len(sizes))
    q = near(rng, base, 300, 4)
    qv = (rng.random(300) < 0.9).astype(np.uint8)
    both_entries(ctx, ops, pair, P, 100, q, what="plain %g" % thr)
    both_entries(ctx, ops, pair, P, 100, q, qv, what="valid %g" % thr)


def test_query_sizes(env):
    ctx, ops, _ = env
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, (32, 32), dtype=np.uint8)
    pair = Pair(ctx, ops)
    for gid in range(3):
        pair.add(gid, near(rng, base, 40 + gid, 8))
    P = ops.place_params(dict(maximum_descriptor_distance=30.0, minimum_age_difference_to_candidates=0, relocalize_min_inliers=2))
    qs = {n: near(rng, base, n, 8) for n in (0, 1, 64, 65, 256, 257, 65536)}
    for n, q in qs.items():
        both_entries(ctx, ops, pair, P, 50, q, what="n_query %d" % n)
    items = [(50 + i, q) for i, q in enumerate(qs.values())]
    got = batch_query(ctx, ops, pair, P, items)
    for (gid, q), g in zip(items, got):
        assert_same(g, pair.ref.query(cparams(P), gid, q), "batch n %d" % len(q))


def test_requery_add_after_query_and_growth(env):
    ctx, ops, _ = env
    rng = np.random.default_rng(4)
    base = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    pair = Pair(ctx, ops)
    pair.dev.reserve(2, 32)
    P = ops.place_params(dict(maximum_descriptor_distance=20.0, minimum_age_difference_to_candidates=1, relocalize_min_inliers=3))
    maps = [near(rng, base, 100 + 37 * i, 3) for i in range(6)]
    for gid, d in enumerate(maps):
        both_entries(ctx, ops, pair, P, 10 * gid, d, what="before add %d" % gid)
        pair.add(10 * gid, d)  # add after query; grows past the reserve
    assert pair.dev.size()[0] == 6
    for gid in (0, 20, 50):  # re-query of stored graph ids: the age rule wraps for newer references
        want = both_entries(ctx, ops, pair, P, gid, maps[gid // 10], what="requery %d" % gid)
        iq = gid // 10
        assert all(c > iq or iq - c > 1 for c in want["candidates"])
    got = batch_query(ctx, ops, pair, P, [(20, maps[2]), (77, maps[2])])
    assert got[0]["index_query"] == 2 and got[1]["index_query"] == 6
    pair.dev.clear()
    assert pair.dev.size() == (0, 0, 0)


def test_capacity_and_bad_queries_in_a_good_batch(env):
    ctx, ops, _ = env
    rng = np.random.default_rng(6)
    base = rng.integers(0, 256, (32, 32), dtype=np.uint8)
    pair = Pair(ctx, ops)
    for gid in range(7):
        pair.add(gid, near(rng, base, 50, 5))
    P = ops.place_params(dict(maximum_descriptor_distance=30.0, minimum_age_difference_to_candidates=0, relocalize_min_inliers=0),
                         max_candidates=4)
    good = near(rng, base, 80, 5)
    q = ops.PlaceQueries(0, 4, 80, 4, pair.dev)
    q.upload(0, 100, good)
    q.upload(1, -5, good)            # negative graph id: PRS_ERR_RANGE
    q.upload(2, 101, good[:0])       # empty: the reference's warning
    q.upload(3, 102, good)
    q.n_query[3] = 81                # above query_stride: PRS_ERR_CAPACITY
    ops.place_query_batch(ctx, pair.dev, P, q)
    ctx.synchronize()
    r = [q.result_of(b, 7) for b in range(4)]
    want = pair.ref.query(cparams(P), 100, good)
    assert want["status"] == pr.ERR_CAPACITY and len(want["candidates"]) == 4  # seven pass, four slots
    assert_same(r[0], want, "overflow")
    assert r[1]["status"] == _lib.ERR_RANGE and r[1]["candidates"] == []
    assert r[2]["status"] == _lib.WARN_EMPTY_INPUT and r[2]["candidates"] == []
    assert r[3]["status"] == _lib.ERR_CAPACITY and r[3]["candidates"] == []
    with pytest.raises(_lib.ProslamHipError):
        pair.dev.query(P, 100, good)  # the host entry reports the overflow as an error


def test_random_database_512_maps(env):
    ctx, ops, _ = env
    rng = np.random.default_rng(12)
    pair = Pair(ctx, ops)
    maps = [rng.integers(0, 256, (2000, 32), dtype=np.uint8) for _ in range(512)]
    for gid, d in enumerate(maps):
        pair.add(gid, d)
    P = ops.place_params(dict(maximum_descriptor_distance=60.0, minimum_age_difference_to_candidates=0, relocalize_min_inliers=20),
                         max_candidates=8)
    items = [(1000 + i, np.concatenate([near(rng, maps[m], 60, 20), rng.integers(0, 256, (200, 32), dtype=np.uint8)]))
             for i, m in enumerate((3, 300, 511))]
    got = batch_query(ctx, ops, pair, P, items)
    for (gid, q), g in zip(items, got):
        want = pair.ref.query(cparams(P), gid, q)
        assert len(want["candidates"]) >= 1
        assert_same(g, want, "random %d" % gid)


def test_captured_graph_replay(env):
    import torch
    ctx, ops, _ = env
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    pair = Pair(ctx, ops)
    for gid in range(5):
        pair.add(gid, near(rng, base, 70 + gid, 6))
    P = ops.place_params(dict(maximum_descriptor_distance=30.0, minimum_age_difference_to_candidates=1, relocalize_min_inliers=4))
    qa, qb = near(rng, base, 90, 6), near(rng, base, 90, 9)
    q = ops.PlaceQueries(0, 2, 90, P.max_candidates, pair.dev)
    q.upload(0, 7, qa)
    q.upload(1, 2, qb)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        ops.place_query_batch(ctx, pair.dev, P, q)  # warm-up on the capture stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ops.place_query_batch(ctx, pair.dev, P, q)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    for swap in (False, True):
        a, b = (qb, qa) if swap else (qa, qb)
        q.upload(0, 7, a)
        q.upload(1, 2, b)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert_same(q.result_of(0, 5), pair.ref.query(cparams(P), 7, a), "replay 0")
        assert_same(q.result_of(1, 5), pair.ref.query(cparams(P), 2, b), "replay 1")


def test_loop_detector_batch_on_the_closures(env):
    ctx, ops, B = env
    sc = {s["name"]: s for s in par.scenarios(B)}
    # KITTI: map 0 = city 00; queries: city 00 (copy) and city 01 -> one candidate each, accepted
    k = configs.get("kitti")
    db = ops.PlaceDatabase(ctx)
    s0 = sc["kitti_00_00"]
    db.add(0, s0["moving_desc"], s0["moving"])
    P = ops.place_params(k["place"], max_candidates=2, minimum_age_difference_to_candidates=0)
    unrelated = [u for u in par.unrelated(B) if u["config"] == "kitti"]
    qs = [sc["kitti_00_00"], sc["kitti_00_01"]]
    det = ops.LoopDetectorBatch(0, db, len(qs) + 1, max(len(q["fixed"]) for q in qs + unrelated[:1]), 2)
    for b, q in enumerate(qs):
        det.upload(b, 1 + b, q["fixed_desc"], q["fixed"])
    det.upload(2, 9, unrelated[0]["fixed_desc"], unrelated[0]["fixed"])  # highway 274: no candidate against city 00
    det.run(ctx, P, ops.bruteforce_params(k["loop"]["maximum_descriptor_distance"], 0.9), ops.point_align_params(k["loop"]))
    ctx.synchronize()
    for b, q in enumerate(qs):
        r = det.result_of(b)
        assert r["candidates"] == [0] and r["accepted"] == [1], (q["name"], r["accepted"])
        err = par.pose_error(r["poses"][0], np.eye(4) if q["truth"] is None else q["truth"])
        assert (np.abs(err) < (np.asarray(q["bounds"]) if q["bounds"] else 1e-5)).all(), q["name"]
    assert det.result_of(2)["candidates"] == [] and int(det.closures.clouds.n_fixed[4].item()) == 0
    # ICL: maps 00 and 01; query 01 -> [0] at 35 bits, query 50 -> [0, 1] at 75 bits
    icl = configs.get("icl")
    db2 = ops.PlaceDatabase(ctx)
    s01 = sc["icl_00_01"]
    db2.add(0, s01["moving_desc"], s01["moving"])
    for dist, b_q, expect in ((35.0, s01, [s01]), (75.0, sc["icl_00_50"], [sc["icl_00_50"], sc["icl_01_50"]])):
        if b_q is not s01:
            db2.add(1, s01["fixed_desc"], s01["fixed"])
        P = ops.place_params(icl["place"], max_candidates=2, minimum_age_difference_to_candidates=0, maximum_descriptor_distance=dist)
        det = ops.LoopDetectorBatch(0, db2, 1, len(b_q["fixed"]), 2)
        det.upload(0, 5, b_q["fixed_desc"], b_q["fixed"])
        det.run(ctx, P, ops.bruteforce_params(dist, 0.9), ops.point_align_params(icl["loop"]))
        ctx.synchronize()
        r = det.result_of(0)
        assert r["candidates"] == list(range(len(expect))) and r["accepted"] == [1] * len(expect), r
        for X, s in zip(r["poses"], expect):
            assert (np.abs(par.pose_error(X, s["truth"])) < np.asarray(s["bounds"])).all(), s["name"]
    # the unrelated ICL query against KITTI city 00
    u = [x for x in par.unrelated(B) if x["config"] == "icl"][0]
    db3 = ops.PlaceDatabase(ctx)
    db3.add(0, u["moving_desc"], u["moving"])
    det = ops.LoopDetectorBatch(0, db3, 1, len(u["fixed"]), 2)
    det.upload(0, 1, u["fixed_desc"], u["fixed"])
    det.run(ctx, ops.place_params(icl["place"], max_candidates=2, minimum_age_difference_to_candidates=0),
            ops.bruteforce_params(35.0, 0.9), ops.point_align_params(icl["loop"]))
    ctx.synchronize()
    assert det.result_of(0)["candidates"] == []


def test_plugin_adapter(env):
    ctx, ops, B = env
    exe = os.path.join(ROOT, "tests", "cpp", "test_place_plugin")
    assert os.path.exists(exe), "build() did not produce the adapter test program"
    case = pr.recognition_3d(B)[1]  # KITTI 00 -> 01, threshold 50, 50 inliers
    tmp = tempfile.mkdtemp()
    fa, fb, fo = (os.path.join(tmp, "place_plugin_%s.bin" % n) for n in ("a", "b", "out"))
    np.asarray(case["ref"], np.uint8).tofile(fa)
    np.asarray(case["query"], np.uint8).tofile(fb)
    out = subprocess.run([exe, fa, str(len(case["ref"])), fb, str(len(case["query"])), fo], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.fromfile(fo, dtype=pr.CORR_DTYPE)
    db = pr.Database()
    db.add(0, case["ref"])
    want = db.query(pr.params(50.0, 0, 50), 1, case["query"])
    assert "indices 1 0" in out.stdout
    assert np.array_equal(got, want["corr"][0])
