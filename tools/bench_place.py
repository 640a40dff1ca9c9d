"""Loop detector candidate search timing (prs_place_query_batch, ops.LoopDetectorBatch): ms per launch by HIP events after warm-up.

  python tools/bench_place.py [--reps 5] [--maps 1,16,256,1024,4096]

Query time against database size: M maps of 1500 descriptors each -- real KITTI ORB rows (the oracle extractor's features of frames
00 and 01 at FAST 5, target 1000, 3 x 3 bins, replicated) or uniform random rows -- searched by B = 1 and B = 64 queries of 1500 rows
(real: the features of frame 01, so that every stored map matches like a revisited place).  Reports descriptor pairs per second and
their fraction of the dense I8 MFMA rate (512 integer operations per pair: 16 x 16 x 256 multiply-adds per tile of 256 pairs).  The
search is exhaustive: its time grows linearly with the database, where a tree would be sublinear.  Last rows: the chained detector
(search, gather, brute-force matcher, loop aligner) in ms per query with up to 8 candidates per query.

  python tools/bench_place.py --bank [--reps 5] [--batches 1,64,1024] [--maps 16,64] [--rows random]

The place bank (prs_place_bank_*, ops.BankDetectorBatch): B sequences with M stored maps of 1500 rows EACH.
  bank_query   prs_place_bank_query_batch alone (init, score, select), by HIP events: pairs per second over B * 1500 * M * 1500 pairs,
               next to prs_place_query_batch of the same build against ONE shared database of M maps (the same pair count).
               tools/ab_place.sh repeats both against a build of the parent commit.
  bank_step    one step captured once and replayed: query + gather + brute-force matcher + loop aligner + append, ms per replay.
               Every replay stores one more map per sequence, so the bank grows from M to M + reps + 3 maps while it is timed.
  early exit   bank_query again with arenas of 64 maps that hold 16 or 1: the score grid is sized by capacity, so most of its
               workgroups return at once.
  route        B = 64, what the bank replaces: device synchronise, copy-back of the hand-over slots, prs_place_db_add per split
               sequence, prs_place_query_batch -- host clock around a step that ends in a synchronise -- next to the bank's query +
               append over the same slots.  A different route, not an A/B of one kernel.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

I8_OPS_PER_S = 5.05e15  # dense v_mfma_i32_16x16x64_i8 rate of the MI355X (2.12 POP/s = 0.42 of it)
ROWS = 1500


def timed(fn, reps):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def real_rows(B):
    import place_ref as pr
    d0, d1 = pr.features_2d(B, "kitti_00"), pr.features_2d(B, "kitti_01")
    return np.concatenate([d0, d1])[:ROWS], np.concatenate([d1, d0])[:ROWS]


PADDED = (ROWS + 15) // 16 * 16


def fill_bank(bank, queries, rows, M):
    """M maps of `rows` in every sequence, stored by the device append from the query slots"""
    import torch
    queries.desc[:, :ROWS] = torch.from_numpy(rows).to(queries.desc.device)
    queries.n_query.fill_(ROWS)
    for m in range(M):
        queries.graph_id.fill_(m)
        bank.append(queries)


def set_queries(queries, qrows, first_id=10**6):
    import torch
    queries.desc[:, :ROWS] = torch.from_numpy(qrows).to(queries.desc.device)
    queries.n_query.fill_(ROWS)
    queries.graph_id.fill_(first_id)


def bank_query(ctx, ops, P, kind, rows, qrows, B, M, reps, capacity=None):
    """the bank's query entry, and the old entry of this build against one shared database of M maps.  capacity: maps the arenas
    have room for (default M: a full bank); with M below it the score grid, sized by capacity, is mostly workgroups that return at once"""
    import torch
    cap = capacity or M
    bank = ops.PlaceBank(ctx, B, cap, cap * PADDED)
    q = ops.PlaceQueries(0, B, ROWS, P.max_candidates, None, count_stride=cap, key_stride=cap * PADDED, corr_stride=ROWS)
    fill_bank(bank, q, rows, M)
    set_queries(q, qrows)
    ms = timed(lambda: ops.place_bank_query_batch(ctx, bank, P, q), reps)
    status = sorted(set(q.status.cpu().numpy().tolist()))
    assert bank.sizes()[0].tolist() == [M] * B
    bank.close()
    del q, bank
    torch.cuda.empty_cache()
    db = ops.PlaceDatabase(ctx)
    db.reserve(M, M * PADDED)
    for m in range(M):
        db.add(m, rows)
    q = ops.PlaceQueries(0, B, ROWS, P.max_candidates, db)
    set_queries(q, qrows)
    ms_shared = timed(lambda: ops.place_query_batch(ctx, db, P, q), reps)
    db.close()
    del q
    torch.cuda.empty_cache()
    pairs = float(B) * ROWS * M * ROWS
    slices = lambda n: (n * PADDED + 1023) // 1024
    print(json.dumps({"object": "bank_query", "rows": kind, "maps": M, "capacity_maps": cap, "batch": B,
                      "score_workgroups_working_of_launched": "%d of %d" % (slices(M) * 6 * B, slices(cap) * 6 * B),
                      "ms_per_launch": round(ms, 4),
                      "pairs_per_s": pairs / (ms * 1e-3), "shared_db_ms_per_launch": round(ms_shared, 4),
                      "shared_db_pairs_per_s": pairs / (ms_shared * 1e-3), "bank_over_shared_time": round(ms / ms_shared, 4),
                      "fraction_of_i8_rate": pairs / (ms * 1e-3) * 512 / I8_OPS_PER_S, "status": status}), flush=True)


def bank_step(ctx, ops, P, mp, ap_, kind, rows, qrows, xyz, B, M, reps):
    """query + gather + matcher + aligner + append, captured once on a side stream and replayed"""
    import torch
    grow = reps + 3  # the warm-up, two replays before the clock and the timed ones each store a map
    bank = ops.PlaceBank(ctx, B, M + grow, (M + grow) * PADDED)
    maxc = P.max_candidates
    det = ops.BankDetectorBatch(0, bank, B, ROWS, maxc, candidate_capacity=0)
    det.queries.xyz[:, :ROWS, :3] = torch.from_numpy(xyz).to(det.queries.xyz.device)
    fill_bank(bank, det.queries, rows, M)
    set_queries(det.queries, qrows)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ctx.use_torch_stream()
        det.run(ctx, P, mp, ap_)  # warm-up on the capture stream: sizes the matcher's work arenas
        det.queries.graph_id.add_(1)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            det.run(ctx, P, mp, ap_)
            det.queries.graph_id.add_(1)
    torch.cuda.current_stream().wait_stream(s)
    ctx.use_torch_stream()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / reps
    maps = bank.sizes()[0]
    print(json.dumps({"object": "bank_step", "rows": kind, "maps_at_start": M, "maps_at_end": int(maps.min()), "batch": B,
                      "max_candidates": maxc, "ms_per_step": round(ms, 4), "ms_per_sequence": round(ms / B, 5),
                      "append_status": sorted(set(bank.append_status.cpu().numpy().tolist())),
                      "candidates_per_query": float(det.queries.n_candidates.float().mean().item())}), flush=True)
    assert int(maps.min()) == int(maps.max()) == M + grow
    bank.close()
    del det, bank, g
    torch.cuda.empty_cache()


def route(ctx, ops, P, kind, rows, qrows, xyz, M, splits, reps):
    """B = 64: the host route (synchronise, copy the hand-over slots back, add per split sequence, query) and the bank's (query,
    append), ms per step by the host clock around steps that end in a synchronise; `splits` sequences hand a map over per step"""
    import time
    import torch
    B = 64
    slots = ops.PlaceQueries(0, B, ROWS, P.max_candidates, None, count_stride=M + (reps + 2) * splits, key_stride=(M + (reps + 2) * splits) * PADDED,
                             corr_stride=ROWS)
    db = ops.PlaceDatabase(ctx)
    db.reserve(M + (reps + 2) * splits, (M + (reps + 2) * splits) * PADDED)
    for m in range(M):
        db.add(m, rows, xyz)
    set_queries(slots, qrows)
    slots.xyz[:, :ROWS, :3] = torch.from_numpy(xyz).to(slots.xyz.device)
    slots.n_query[splits:] = 0
    next_id = [10**6]

    def host_step():
        ctx.synchronize()
        n = slots.n_query.cpu().numpy()
        ids = slots.graph_id.cpu().numpy()
        d, x = slots.desc.cpu().numpy(), slots.xyz.cpu().numpy()
        ops.place_query_batch(ctx, db, P, slots)  # query, then add: a map never matches itself
        ctx.synchronize()
        for b in np.flatnonzero(n > 0):
            db.add(next_id[0], d[b, : n[b]], x[b, : n[b], :3])
            next_id[0] += 1
        del ids

    for _ in range(2):
        host_step()
    t0 = time.perf_counter()
    for _ in range(reps):
        host_step()
    ctx.synchronize()
    ms_host = (time.perf_counter() - t0) * 1e3 / reps
    db.close()
    bank = ops.PlaceBank(ctx, B, M + reps + 2, (M + reps + 2) * PADDED)
    q = ops.PlaceQueries(0, B, ROWS, P.max_candidates, None, count_stride=M + reps + 2, key_stride=(M + reps + 2) * PADDED, corr_stride=ROWS)
    fill_bank(bank, q, rows, M)
    set_queries(q, qrows)
    q.n_query[splits:] = 0

    def bank_step_():
        ops.place_bank_query_batch(ctx, bank, P, q)
        bank.append(q)
        q.graph_id.add_(1)

    for _ in range(2):
        bank_step_()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        bank_step_()
    ctx.synchronize()
    ms_bank = (time.perf_counter() - t0) * 1e3 / reps
    print(json.dumps({"object": "route", "rows": kind, "batch": B, "maps_at_start": M, "splits_per_step": splits,
                      "host_route_ms_per_step": round(ms_host, 3), "bank_route_ms_per_step": round(ms_bank, 3),
                      "note": "host route: ONE shared database that grows by `splits` maps a step; bank: per-sequence, one map a step"}),
          flush=True)
    bank.close()
    del q, slots, bank
    torch.cuda.empty_cache()


def main_bank(args):
    import torch
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import configs, ops
    ctx = ops.Context(0)
    rng = np.random.default_rng(0)
    kinds = {}
    for kind in args.rows.split(","):
        if kind == "kitti":
            from test_ref_pins import OracleBackend
            kinds[kind] = real_rows(OracleBackend())
        else:
            kinds[kind] = (rng.integers(0, 256, (ROWS, 32), dtype=np.uint8), rng.integers(0, 256, (ROWS, 32), dtype=np.uint8))
    k = configs.get("kitti")
    xyz = rng.uniform(-10, 10, (ROWS, 3)).astype(np.float32) + np.float32([0, 0, 20])
    mp, ap_ = ops.bruteforce_params(k["loop"]["maximum_descriptor_distance"], 0.9), ops.point_align_params(k["loop"])
    batches, maps = [int(x) for x in args.batches.split(",")], [int(x) for x in args.maps.split(",")]
    sections = args.sections.split(",")
    for kind, (rows, qrows) in kinds.items():
        P = ops.place_params(k["place"], max_candidates=8, minimum_age_difference_to_candidates=0)
        for M in maps:
            for B in batches:
                if "query" in sections:
                    bank_query(ctx, ops, P, kind, rows, qrows, B, M, args.reps)
                # 8 candidate slots per query up to B = 64, 2 at B = 1024 (the pair slots are B * slots clouds of 1500 points)
                Ps = ops.place_params(k["place"], max_candidates=8 if B <= 64 else 2, minimum_age_difference_to_candidates=0)
                if "step" in sections:
                    bank_step(ctx, ops, Ps, mp, ap_, kind, rows, qrows, xyz, B, M, args.reps)
        if "early" in sections:
            for M in (16, 1):
                for B in batches:
                    bank_query(ctx, ops, P, kind, rows, qrows, B, M, args.reps, capacity=64)
        if "route" in sections:
            for splits in (64, 8):
                route(ctx, ops, P, kind, rows, qrows, xyz, maps[0], splits, args.reps)
    torch.cuda.synchronize()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--maps", default=None)
    ap.add_argument("--bank", action="store_true", help="the place bank: query entry, captured step, and the host route it replaces")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--rows", default="random")
    ap.add_argument("--sections", default="query,step,early,route", help="with --bank: which measurements to take")
    args = ap.parse_args()
    if args.bank:
        args.maps = args.maps or "16,64"
        return main_bank(args)
    args.maps = args.maps or "1,16,256,1024,4096"
    import torch
    import __graft_entry__ as g
    g.build()
    from srrg2_proslam_amd import configs, ops
    from test_ref_pins import OracleBackend
    ctx = ops.Context(0)
    stored, query = real_rows(OracleBackend())
    rng = np.random.default_rng(0)
    rand = rng.integers(0, 256, (ROWS, 32), dtype=np.uint8)
    place = configs.get("kitti")["place"]
    P = ops.place_params(place, max_candidates=8, minimum_age_difference_to_candidates=0)
    for kind, rows, qrows in (("kitti", stored, query), ("random", rand, rng.integers(0, 256, (ROWS, 32), dtype=np.uint8))):
        db = ops.PlaceDatabase(ctx)
        n_maps = 0
        for M in [int(x) for x in args.maps.split(",")]:
            db.reserve(M, M * ROWS)
            while n_maps < M:
                db.add(n_maps, rows)
                n_maps += 1
            for B in (1, 64):
                q = ops.PlaceQueries(0, B, ROWS, P.max_candidates, db)
                for b in range(B):
                    q.upload(b, 10**6 + b, qrows)
                ms = timed(lambda: ops.place_query_batch(ctx, db, P, q), args.reps)
                pairs = float(B) * ROWS * M * ROWS
                rate = pairs / (ms * 1e-3)
                print(json.dumps({"object": "place_query", "rows": kind, "maps": M, "batch": B, "ms_per_launch": round(ms, 4),
                                  "ms_per_query": round(ms / B, 4), "pairs_per_s": rate, "fraction_of_i8_rate": rate * 512 / I8_OPS_PER_S,
                                  "status": sorted(set(q.status.cpu().numpy().tolist()))}), flush=True)
                del q
                torch.cuda.empty_cache()
        db.close()
    # the chained detector on real rows: 256 stored maps, every one a candidate (8 slots per query)
    k = configs.get("kitti")
    db = ops.PlaceDatabase(ctx)
    xyz = rng.uniform(-10, 10, (ROWS, 3)).astype(np.float32) + np.float32([0, 0, 20])
    for m in range(256):
        db.add(m, stored, xyz)
    for B in (1, 16):
        det = ops.LoopDetectorBatch(0, db, B, ROWS, 8, candidate_capacity=0)
        for b in range(B):
            det.upload(b, 10**6 + b, query, xyz)
        mp, ap_ = ops.bruteforce_params(k["loop"]["maximum_descriptor_distance"], 0.9), ops.point_align_params(k["loop"])
        ms = timed(lambda: det.run(ctx, P, mp, ap_), args.reps)
        print(json.dumps({"object": "loop_detector_chain", "maps": 256, "batch": B, "candidates_per_query": 8, "ms_per_launch": round(ms, 4),
                          "ms_per_query": round(ms / B, 4)}), flush=True)
        del det
    db.close()
    ctx.close()


if __name__ == "__main__":
    main()
