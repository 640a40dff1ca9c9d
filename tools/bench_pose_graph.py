"""Pose-graph optimiser timing (prs_pose_graph_optimize_batch / prs_pose_graph_optimize_lm_batch): graphs per second and ms per
Gauss-Newton iteration or Levenberg-Marquardt round by HIP events.

  python tools/bench_pose_graph.py [--algorithm gn|lm] [--reps 3] [--batches 1,64,1024] [--iterations 4] [--steps 40,10]
                                   [--perturb TS,QS]

The graphs are cut from KITTI-00 ground truth (tests/pose_graph_cases.py kitti_case): every 40th pose (114 nodes, 125 edges, 12
closures, 1064 envelope blocks) and every 10th (455 nodes, 537 edges, 83 closures, 22410 blocks), the same graph in every slot of
the batch, the criterion off so that every graph runs `--iterations` iterations.  Per graph size it prints
  parity   the device result against the dense float64 reference (tests/pose_graph_ref.py optimize_dense), max |dt| and |dq|;
  cpu      the same-box baseline: the independent reference's linearisation with scipy.sparse.linalg.spsolve, ms per iteration;
  B = ...  ms per launch, graphs per second and ms per iteration (launch time / iterations; the error-only pass is inside).
--algorithm lm runs the shipped icl / tum parameters (100 trials, tau 1e-5, clamps 1/3 and 2/3, variable damping) for `--iterations`
rounds and adds the trials of every round to each row; from their own guess the KITTI graphs accept every first trial, so a round
is a Gauss-Newton iteration plus the error pass and the `scale` sum.  --perturb TS,QS right-multiplies every free node's guess by a
seeded random pose (sigma TS metres, QS quaternion units, seed 7): trials are rejected, and the launch time less the rounds' share
is what the rejected trials cost (a linearisation, a factorisation and an error pass each).  The parity and cpu rows belong to the
Gauss-Newton run and are skipped for lm.
One JSON line per row.  B = 1 is one wave on a dependency chain: expect it to lose to the CPU solver; the case for the kernel is B
graphs per launch with the closures never leaving the device.
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


def cpu_iteration_ms(c, reps):
    """one Gauss-Newton iteration on the CPU: vectorised linearisation, scipy sparse assembly, spsolve, update"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    import pose_graph_ref as ref
    X = c["poses"].copy()
    n, src, dst = len(X), c["src"], c["dst"]
    free = c["fixed"] == 0
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        e, Jf, Jt = ref.edge_terms(X[src], X[dst], c["Z"])
        blocks = [(src, src, np.einsum("eka,ekb->eab", Jf, Jf)), (dst, dst, np.einsum("eka,ekb->eab", Jt, Jt)),
                  (dst, src, np.einsum("eka,ekb->eab", Jt, Jf)), (src, dst, np.einsum("eka,ekb->eab", Jf, Jt))]
        rows = np.concatenate([(6 * r[:, None, None] + np.arange(6)[None, :, None] + np.zeros((1, 1, 6), int)).reshape(-1) for r, _, _ in blocks])
        cols = np.concatenate([(6 * q[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), int)).reshape(-1) for _, q, _ in blocks])
        H = sp.coo_matrix((np.concatenate([v.reshape(-1) for _, _, v in blocks]), (rows, cols)), shape=(6 * n, 6 * n)).tocsr()
        b = np.zeros(6 * n)
        np.add.at(b, (6 * src[:, None] + np.arange(6)).reshape(-1), np.einsum("eka,ek->ea", Jf, e).reshape(-1))
        np.add.at(b, (6 * dst[:, None] + np.arange(6)).reshape(-1), np.einsum("eka,ek->ea", Jt, e).reshape(-1))
        keep = np.repeat(free, 6)
        H = H[keep][:, keep]
        H = (H + 1e-6 * sp.diags(H.diagonal())).tocsc()
        dx = np.zeros(6 * n)
        dx[keep] = spl.spsolve(H, -b[keep])
        Xn = X.copy()
        Xn[free] = ref.se3_mul(X[free], ref.tnq2t(dx.reshape(n, 6)[free]))
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--steps", default="40,10")
    ap.add_argument("--algorithm", choices=("gn", "lm"), default="gn")
    ap.add_argument("--perturb", default="")
    args = ap.parse_args()
    lm = args.algorithm == "lm"
    import torch
    import __graft_entry__ as g
    g.build()
    import pose_graph_cases as pc
    import pose_graph_ref as ref
    from srrg2_proslam_amd import configs, ops
    ctx = ops.Context(0)
    if lm:
        P = ops.pose_graph_lm_params(configs.get("icl")["graph"], max_iterations=args.iterations, epsilon=0.0)
    else:
        P = ops.pose_graph_params(dict(damping=1e-6, max_iterations=args.iterations, epsilon=0.0))
    run = ops.pose_graph_optimize_lm_batch if lm else ops.pose_graph_optimize_batch
    for step in (int(s) for s in args.steps.split(",")):
        c = pc.kitti_case(step=step)
        n, E = len(c["poses"]), len(c["src"])
        blocks = ops.pose_graph_envelope_blocks(n, c["src"], c["dst"])
        if args.perturb:
            ts, qs = (float(v) for v in args.perturb.split(","))
            rng = np.random.default_rng(7)
            c = dict(c, poses=c["poses"].copy())
            for i in range(n):
                if not c["fixed"][i]:
                    c["poses"][i] = ref.se3_mul(c["poses"][i], pc._rand_pose(rng, ts, qs))
        if not lm:
            bench_parity_and_cpu(args, ctx, ops, pc, ref, P, c, n, E, blocks)
        for B in (int(s) for s in args.batches.split(",")):
            graphs = ops.PoseGraphBatch(0, B, n, E, blocks, with_omega=False, lm=lm)
            graphs.upload(0, c["poses"], c["fixed"], (c["src"], c["dst"], c["Z"]))
            for t in (graphs.X, graphs.fixed, graphs.src, graphs.dst, graphs.Z):
                t[1:] = t[0]
            graphs.n_nodes[:], graphs.n_edges[:] = n, E
            start = graphs.X.clone()
            ms = []
            for rep in range(args.reps + 1):  # the first launch is the warm-up
                graphs.X.copy_(start)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(ctx, P, graphs)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            r = graphs.lm_result_of(B - 1) if lm else graphs.result_of(B - 1)
            assert r["status"] == 0 and (args.perturb or r["iterations"] == args.iterations), r
            assert torch.equal(graphs.X[0], graphs.X[B - 1])
            best = min(ms[1:])
            row = dict(graph=c["name"], algorithm=args.algorithm, row="B=%d" % B, ms_per_launch=best, graphs_per_s=B / best * 1e3,
                       iterations=r["iterations"], ms_per_iteration=best / max(r["iterations"], 1),
                       ms_per_iteration_per_graph=best / max(r["iterations"], 1) / B, chi_0=float(r["chi"][0]), chi_final=float(r["chi_final"]))
            if lm:
                row.update(trials=r["trials"], trials_total=r["trials_total"], stalled=r["stalled"])
            print(json.dumps(row), flush=True)
    ctx.close()


def bench_parity_and_cpu(args, ctx, ops, pc, ref, P, c, n, E, blocks):
    dense = ref.optimize_dense(c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], None, 1e-6, 0, args.iterations, 0.0)
    X, res, _ = ops.pose_graph_optimize(ctx, P, c["poses"], c["fixed"], c["src"], c["dst"], c["Z"])
    dt, dq = pc.pose_difference(X.reshape(-1, 16), dense["X"])
    print(json.dumps(dict(graph=c["name"], nodes=n, edges=E, envelope_blocks=blocks, row="parity", max_dt=dt, max_dq=dq,
                          chi_final=float(res["chi_final"]), chi_final_dense=float(dense["chi_final"]))), flush=True)
    print(json.dumps(dict(graph=c["name"], row="cpu", ms_per_iteration=cpu_iteration_ms(c, args.reps))), flush=True)


if __name__ == "__main__":
    main()
