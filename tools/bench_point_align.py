"""Loop aligner timing (prs_point_align_batch): ms per launch by HIP events after warm-up, and registrations per second.

  python tools/bench_point_align.py [--reps 20]

Rows: KITTI settings (100 iterations, the 00 -> 01 pair, 43 correspondences) and ICL settings (10 iterations, the 00 -> 01 pair,
219 correspondences) replicated to B = 1, 16, 256, 1024, 4096; a synthetic 2000-correspondence pair; the brute-force match +
registration chain on the real pairs; one pair through the host entry.  Kernel times: run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_point_align.py` separately.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import point_align_ref as par
    from oracle import binding as ob
    from srrg2_proslam_amd import configs, ops
    from test_ref_pins import OracleBackend
    ctx = ops.Context(0)
    sc = {s["name"]: s for s in par.scenarios(OracleBackend())}
    rows = []
    for cfg, name, dist in (("kitti", "kitti_00_01", 25.0), ("icl", "icl_00_01", 35.0)):
        s = sc[name]
        corr, _ = ob.bruteforce_match(s["fixed_desc"], s["moving_desc"], dist, 0.9)
        P = ops.point_align_params(configs.get(cfg)["loop"])
        for B in (1, 16, 256, 1024, 4096):
            pb = ops.PointAlignBatch(0, B, len(s["fixed"]), len(s["moving"]), max(len(corr), 1), with_mask=False)
            pb.upload(0, s["fixed"], s["moving"], corr)
            for t in (pb.fixed, pb.moving, pb.corr, pb.n_fixed, pb.n_moving, pb.n_corr, pb.X):
                t[1:] = t[0]
            ms = timed(lambda: ops.point_align_batch(ctx, P, pb), args.reps)
            rows.append(dict(row="%s_B%d" % (cfg, B), n_corr=len(corr), iterations=P.max_iterations, ms=round(ms, 4),
                             registrations_per_s=round(B / ms * 1e3)))
        lc = ops.LoopClosureBatch(0, 256, len(s["fixed"]), len(s["moving"]), with_mask=False,
                                  candidate_capacity=len(s["fixed"]) * len(s["moving"]))
        for b in range(256):
            lc.upload(b, s["fixed"], s["fixed_desc"], s["moving"], s["moving_desc"])
        ms = timed(lambda: lc.run(ctx, ops.bruteforce_params(dist, 0.9), P), args.reps)
        rows.append(dict(row="%s_match_register_B256" % cfg, ms=round(ms, 4), registrations_per_s=round(256 / ms * 1e3)))
        t0 = time.perf_counter()
        for _ in range(args.reps):
            ops.point_align(ctx, P, s["fixed"], s["moving"], corr, np.eye(4), with_mask=False)
        rows.append(dict(row="%s_host_entry_B1" % cfg, ms=round((time.perf_counter() - t0) / args.reps * 1e3, 4)))
    rng = np.random.default_rng(1)
    moving = rng.uniform(-20, 20, (2000, 3)).astype(np.float32)
    fixed = moving + rng.normal(0, 0.02, moving.shape).astype(np.float32)
    corr = np.stack([np.arange(2000), np.arange(2000)], 1).astype(np.int32)
    P = ops.point_align_params(configs.get("kitti")["loop"])
    for B in (1, 256):
        pb = ops.PointAlignBatch(0, B, 2000, 2000, 2000, with_mask=False)
        pb.upload(0, fixed, moving, corr)
        for t in (pb.fixed, pb.moving, pb.corr, pb.n_fixed, pb.n_moving, pb.n_corr, pb.X):
            t[1:] = t[0]
        ms = timed(lambda: ops.point_align_batch(ctx, P, pb), args.reps)
        rows.append(dict(row="synthetic_2000_B%d" % B, iterations=100, ms=round(ms, 4), registrations_per_s=round(B / ms * 1e3)))
    for r in rows:
        print(json.dumps(r))
    ctx.close()


if __name__ == "__main__":
    main()
