"""The loop detector's kernels (csrc/place_db.hip) on the planted cases of tests/place_cases.py: every query through the batch entry
and, where its status is no error, through prs_place_query, bit for bit against the CPU checker; prs_place_gather_pairs called
directly and compared array for array with place_ref.gather_pairs.  tests/test_place_cases.py shows on the CPU what each case
holds: a pair one bit under the threshold and its twin on it in every accumulator slot, planted rows, query rows, ties, counts."""
import ctypes as C

import numpy as np
import pytest

import place_cases as pc
import place_ref as pr
from place_cases import Pair, assert_same, batch_query, both_entries, cparams
from srrg2_proslam_amd import _lib

pytestmark = pytest.mark.gpu
PATTERN = 0x5A


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


def load(ctx, ops, case):
    pair = Pair(ctx, ops)
    for m in case["maps"]:
        pair.add(m["gid"], m["desc"], m["xyz"], m["valid"])
    P = ops.place_params(case["P"], max_candidates=case["P"]["max_candidates"])
    return pair, P


def run_case(ctx, ops, case):
    """every query alone through both entries, then all of them as one batch"""
    pair, P = load(ctx, ops, case)
    want = [both_entries(ctx, ops, pair, P, q["gid"], q["desc"], q["valid"], "%s query %d" % (case["name"], b))
            for b, q in enumerate(case["queries"])]
    if len(want) > 1:
        masked = any(q["valid"] is not None for q in case["queries"])
        got = batch_query(ctx, ops, pair, P, [(q["gid"], q["desc"], q["valid"]) for q in case["queries"]], with_valid=masked)
        for b, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, "%s batch slot %d" % (case["name"], b))
    for key in ("counts", "candidates"):  # the checker's result is the one the case's name promises
        if key in case["claims"]:
            assert [list(map(int, w[key])) for w in want] == case["claims"][key], key
    return pair, P, want


@pytest.mark.parametrize("name", ["slots", "slots_valid"])
def test_boundary_in_every_accumulator_slot(env, name):
    ctx, ops = env
    _, _, want = run_case(ctx, ops, pc.by_name(name))
    c = want[0]["corr"][0]
    assert (c["response"] == pc.LIM - 1).all() and len(c) == want[0]["counts"][0]  # the twins at 33 bits leave no key and no count


@pytest.mark.parametrize("name", ["rows", "queries", "ties", "counts", "age"])
def test_planted_positions(env, name):
    ctx, ops = env
    run_case(ctx, ops, pc.by_name(name))


def test_query_row_65535(env):
    ctx, ops = env
    case = pc.by_name("query_65535")
    pair, P, want = run_case(ctx, ops, case)
    assert 65535 in want[0]["corr"][0]["fixed_idx"]
    q = case["queries"][0]
    full = both_entries(ctx, ops, pair, P, q["gid"], q["desc"], None, "query_65535 without mask")
    assert 65535 in full["corr"][0]["fixed_idx"]


@pytest.mark.parametrize("thr", pc.THRESHOLDS, ids=["%g" % t for t in pc.THRESHOLDS])
def test_thresholds(env, thr):
    ctx, ops = env
    case = pc.by_name("thr_%g" % thr)
    pair, P, want = run_case(ctx, ops, case)
    lim = case["claims"]["thr:%g" % thr]["lim"]
    stored = sum(len(m["desc"]) for m in pair.ref.maps)
    # run_case has compared the device with `want` bit for bit (assert_same); these two lines pin what `want` itself holds
    if lim == 257:  # every stored row matches each of the three query rows, no pad row counts; a real row at 256 bits matches
        assert int(want[0]["counts"].sum()) == 3 * stored and want[1]["corr"][0]["response"][0] == 256.0
    if lim == 0:
        assert int(want[0]["counts"].sum()) == 0


def test_nan_threshold_is_refused(env):
    ctx, ops = env
    case = pc.by_name("thr_33")
    pair, _ = load(ctx, ops, case)
    P = ops.place_params(dict(case["P"], maximum_descriptor_distance=float("nan")))
    q = case["queries"][0]
    with pytest.raises(_lib.ProslamHipError) as e:
        batch_query(ctx, ops, pair, P, [(q["gid"], q["desc"])])
    assert e.value.status == _lib.ERR_RANGE
    with pytest.raises(_lib.ProslamHipError) as e:
        pair.dev.query(P, q["gid"], q["desc"])
    assert e.value.status == _lib.ERR_RANGE


def fill(*tensors):
    import torch
    for t in tensors:
        t.view(torch.uint8).fill_(PATTERN)


def is_pattern(t):
    import torch
    return bool((t.contiguous().view(torch.uint8) == PATTERN).all().item())


def test_strides_and_reuse(env):
    ctx, ops = env
    case = pc.by_name("strides")
    pair, P = load(ctx, ops, case)
    maps, rows, big = pair.dev.size()
    Q = case["queries"]
    qs = max(len(q["desc"]) for q in Q)
    q = ops.PlaceQueries(0, 3, qs, P.max_candidates, pair.dev, count_stride=maps + 3, key_stride=rows + 48, corr_stride=big + 5)
    outputs = (q.match_counts, q.best_keys, q.candidates, q.n_candidates, q.corr, q.n_corr, q.status, q.index_query)
    fill(*outputs)

    def run(items, what):
        for b, (gid, desc) in enumerate(items):
            q.upload(b, gid, desc)
        ops.place_query_batch(ctx, pair.dev, P, q)
        ctx.synchronize()
        n_maps, n_rows, _ = pair.dev.size()
        for b, (gid, desc) in enumerate(items):
            assert_same(q.result_of(b, n_maps), pair.ref.query(cparams(P), gid, desc), "%s slot %d" % (what, b))
        # what lies between the database's size and the strides is not the kernels' to write
        assert is_pattern(q.match_counts[:, n_maps:]) and is_pattern(q.best_keys[:, n_rows:]) and is_pattern(q.corr[:, :, big:])

    first = [(x["gid"], x["desc"]) for x in Q]
    run(first, "first")
    # the slots permuted and cut short, so that each holds fewer matches than the run before left in it
    second = [(Q[2]["gid"], Q[2]["desc"][:19]), (Q[0]["gid"], Q[0]["desc"][:5]), (Q[1]["gid"], Q[1]["desc"][:40])]
    want = [pair.ref.query(cparams(P), gid, desc) for gid, desc in second]
    assert [int(w["counts"].sum()) for w in want] == [2, 1, 2]
    run(second, "second")
    rng = np.random.default_rng(5)
    extra = pc.random_rows(rng, 20)
    extra[7] = Q[0]["desc"][1]
    pair.add(500, extra)  # a fifth map: the strides still suffice
    assert pair.dev.size() == (maps + 1, rows + 32, big)
    run(first, "after add")
    assert 4 in q.result_of(0, maps + 1)["candidates"]
    # each stride one below its need: refused at call level, the outputs untouched
    maps, rows, big = pair.dev.size()
    for short in ("count_stride", "key_stride", "corr_stride"):
        strides = dict(count_stride=maps, key_stride=rows, corr_stride=big)
        strides[short] -= 1
        bad = ops.PlaceQueries(0, 3, qs, P.max_candidates, pair.dev, **strides)
        out = (bad.match_counts, bad.best_keys, bad.candidates, bad.n_candidates, bad.corr, bad.n_corr, bad.status, bad.index_query)
        fill(*out)
        for b, (gid, desc) in enumerate(first):
            bad.upload(b, gid, desc)
        with pytest.raises(_lib.ProslamHipError) as e:
            ops.place_query_batch(ctx, pair.dev, P, bad)
        assert e.value.status == _lib.ERR_CAPACITY, short
        ctx.synchronize()
        assert all(is_pattern(t) for t in out), short


def gather(ctx, ops, case, fixed_extra=0, moving_extra=0):
    """prs_place_query_batch, then prs_place_gather_pairs on pattern-filled pair slots -> (detector, checker results, pair)"""
    import torch
    pair, P = load(ctx, ops, case)
    Q = case["queries"]
    maxc, big = P.max_candidates, pair.dev.size()[2]
    qs = max(max(len(x["desc"]) for x in Q), 1)
    det = ops.LoopDetectorBatch(0, pair.dev, len(Q), qs, maxc, moving_stride=big + moving_extra, with_valid=True)
    if fixed_extra:  # pair slots wider than the query slots: a closure batch of that width, its counts shared between matcher and
        # aligner exactly as LoopDetectorBatch.__init__ wires them (ops.py; keep the two in step)
        det.closures = ops.LoopClosureBatch(0, len(Q) * maxc, qs + fixed_extra, big + moving_extra, with_mask=False, candidate_capacity=1)
        det.closures.pairs.n_fixed, det.closures.pairs.n_moving = det.closures.clouds.n_fixed, det.closures.clouds.n_moving
    for b, x in enumerate(Q):
        det.upload(b, x["gid"], x["desc"], x["xyz"], x["valid"])
    lc = det.closures
    outs = (lc.pairs.fixed, lc.clouds.fixed_desc, lc.clouds.n_fixed, lc.pairs.moving, lc.clouds.moving_desc, lc.clouds.n_moving, lc.pairs.X)
    fill(*outs)
    ops.place_query_batch(ctx, pair.dev, P, det.queries)
    qd, pd = det.queries.descriptor(), det.pairs_descriptor()
    assert (pd.fixed_stride, pd.moving_stride) == (qs + fixed_extra, big + moving_extra)
    rc = _lib.load().prs_place_gather_pairs(pair.dev._h, C.byref(P), C.byref(qd), C.byref(pd))
    assert rc == 0
    ctx.synchronize()
    torch.cuda.synchronize()
    want = [pair.ref.query(cparams(P), x["gid"], x["desc"], x["valid"]) for x in Q]
    for b, (x, w) in enumerate(zip(Q, want)):
        assert_same(det.queries.result_of(b, len(pair.ref.maps)), w, "%s query %d" % (case["name"], b))
        slots = pr.gather_pairs(pair.ref, w, x["desc"], x["xyz"], x["valid"], maxc)
        for k, s in enumerate(slots):
            i, what = b * maxc + k, "%s query %d slot %d" % (case["name"], b, k)
            nf, nm = int(lc.clouds.n_fixed[i].item()), int(lc.clouds.n_moving[i].item())
            assert (nf, nm) == (s["n_fixed"], s["n_moving"]), what
            assert (k < len(w["candidates"])) == (nm > 0), what
            for n, xyz, desc, wx, wd in ((nf, lc.pairs.fixed[i], lc.clouds.fixed_desc[i], s["fixed_xyz"], s["fixed_desc"]),
                                        (nm, lc.pairs.moving[i], lc.clouds.moving_desc[i], s["moving_xyz"], s["moving_desc"])):
                got = xyz[:n].cpu().numpy()
                assert np.array_equal(got[:, :3].view(np.uint32), np.ascontiguousarray(wx, np.float32).view(np.uint32)), what
                assert (got[:, 3].view(np.uint32) == 0).all(), what
                assert np.array_equal(desc[:n].cpu().numpy(), wd), what
                assert is_pattern(xyz[n:]) and is_pattern(desc[n:]), what  # rows beyond the count keep the pattern
            assert np.array_equal(lc.pairs.X[i].cpu().numpy().reshape(4, 4), s["X"]), what
    return det, want, pair, P


@pytest.mark.parametrize("name", ["gather_valid", "gather_overflow", "gather_slots_1", "gather_slots_3", "gather_slots_4", "gather_slots_5"])
def test_gather_pairs(env, name):
    ctx, ops = env
    case = pc.by_name(name)
    _, want, _, _ = gather(ctx, ops, case)
    assert [w["candidates"] for w in want] == case["claims"]["candidates"]
    if name == "gather_overflow":
        assert [w["status"] for w in want] == [pr.ERR_CAPACITY, pr.WARN_EMPTY_INPUT, pr.ERR_RANGE, pr.ERR_CAPACITY]


def test_gather_pairs_wider_slots_and_refusals(env):
    ctx, ops = env
    case = pc.by_name("gather_valid")
    det, _, pair, P = gather(ctx, ops, case, fixed_extra=7, moving_extra=9)
    lc = det.closures
    outs = (lc.pairs.fixed, lc.clouds.fixed_desc, lc.clouds.n_fixed, lc.pairs.moving, lc.clouds.moving_desc, lc.clouds.n_moving, lc.pairs.X)
    fill(*outs)
    qd = det.queries.descriptor()
    for field, below in (("fixed_stride", det.queries.query_stride - 1), ("moving_stride", pair.dev.size()[2] - 1)):
        pd = det.pairs_descriptor()
        setattr(pd, field, below)
        rc = _lib.load().prs_place_gather_pairs(pair.dev._h, C.byref(P), C.byref(qd), C.byref(pd))
        assert rc == _lib.ERR_CAPACITY, field
        ctx.synchronize()
        assert all(is_pattern(t) for t in outs), field
