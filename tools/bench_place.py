"""Loop detector candidate search timing (prs_place_query_batch, ops.LoopDetectorBatch): ms per launch by HIP events after warm-up.

  python tools/bench_place.py [--reps 5] [--maps 1,16,256,1024,4096]

Query time against database size: M maps of 1500 descriptors each -- real KITTI ORB rows (the oracle extractor's features of frames
00 and 01 at FAST 5, target 1000, 3 x 3 bins, replicated) or uniform random rows -- searched by B = 1 and B = 64 queries of 1500 rows
(real: the features of frame 01, so that every stored map matches like a revisited place).  Reports descriptor pairs per second and
their fraction of the dense I8 MFMA rate (512 integer operations per pair: 16 x 16 x 256 multiply-adds per tile of 256 pairs).  The
search is exhaustive: its time grows linearly with the database, where a tree would be sublinear.  Last rows: the chained detector
(search, gather, brute-force matcher, loop aligner) in ms per query with up to 8 candidates per query.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--maps", default="1,16,256,1024,4096")
    args = ap.parse_args()
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
