"""Pose-graph optimiser timing (prs_pose_graph_optimize_batch): graphs per second and ms per Gauss-Newton iteration by HIP events.

  python tools/bench_pose_graph.py [--reps 3] [--batches 1,64,1024] [--iterations 4] [--steps 40,10]

The graphs are cut from KITTI-00 ground truth (tests/pose_graph_cases.py kitti_case): every 40th pose (114 nodes, 125 edges, 12
closures, 1064 envelope blocks) and every 10th (455 nodes, 537 edges, 83 closures, 22410 blocks), the same graph in every slot of
the batch, the criterion off so that every graph runs `--iterations` iterations.  Per graph size it prints
  parity   the device result against the dense float64 reference (tests/pose_graph_ref.py optimize_dense), max |dt| and |dq|;
  cpu      the same-box baseline: the independent reference's linearisation with scipy.sparse.linalg.spsolve, ms per iteration;
  B = ...  ms per launch, graphs per second and ms per iteration (launch time / iterations; the error-only pass is inside).
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
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import pose_graph_cases as pc
    import pose_graph_ref as ref
    from srrg2_proslam_amd import ops
    ctx = ops.Context(0)
    P = ops.pose_graph_params(dict(damping=1e-6, max_iterations=args.iterations, epsilon=0.0))
    for step in (int(s) for s in args.steps.split(",")):
        c = pc.kitti_case(step=step)
        n, E = len(c["poses"]), len(c["src"])
        blocks = ops.pose_graph_envelope_blocks(n, c["src"], c["dst"])
        dense = ref.optimize_dense(c["poses"], c["fixed"], c["src"], c["dst"], c["Z"], None, 1e-6, 0, args.iterations, 0.0)
        X, res, _ = ops.pose_graph_optimize(ctx, P, c["poses"], c["fixed"], c["src"], c["dst"], c["Z"])
        dt, dq = pc.pose_difference(X.reshape(-1, 16), dense["X"])
        print(json.dumps(dict(graph=c["name"], nodes=n, edges=E, envelope_blocks=blocks, row="parity", max_dt=dt, max_dq=dq,
                              chi_final=float(res["chi_final"]), chi_final_dense=float(dense["chi_final"]))), flush=True)
        print(json.dumps(dict(graph=c["name"], row="cpu", ms_per_iteration=cpu_iteration_ms(c, args.reps))), flush=True)
        for B in (int(s) for s in args.batches.split(",")):
            graphs = ops.PoseGraphBatch(0, B, n, E, blocks, with_omega=False)
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
                ops.pose_graph_optimize_batch(ctx, P, graphs)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            r = graphs.result_of(B - 1)
            assert r["status"] == 0 and r["iterations"] == args.iterations, r
            assert torch.equal(graphs.X[0], graphs.X[B - 1])
            best = min(ms[1:])
            print(json.dumps(dict(graph=c["name"], row="B=%d" % B, ms_per_launch=best, graphs_per_s=B / best * 1e3,
                                  ms_per_iteration=best / args.iterations, ms_per_iteration_per_graph=best / args.iterations / B)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
