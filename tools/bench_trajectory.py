#!/usr/bin/env python3
"""The trajectory evaluator (ops.TrajectoryEvalBatch: ATE, RPE, the KITTI block, one launch) at B sequences of 4541 rows -- the
KITTI-00 ground truth against seeded drifting copies of it -- beside the host route it replaces: the device-to-host copy of the
estimates (`.cpu()`) plus the float64 numpy restatement (tests/trajectory_ref.py) walking every sequence.

Device time: device events around `reps` launches after a warm-up, median.  Achieved bytes per second: the algorithmic 128 bytes a
row (one float32 pose of each cloud) over that time.  Host route: the copy is timed whole; the numpy walk is timed on `--host-sample`
sequences and scaled to B (it is a per-sequence loop), and says so in its key.

`--breakdown` also times the launch with blocks of the metric switched off (no KITTI block; one length; no alignment; no relative
poses), which prices the kernel's phases by difference.

    python tools/bench_trajectory.py [--batches 1,256,4096] [--rows 4541] [--host-sample 4] [--breakdown]
prints one JSON line.
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

UNIQUE = 4


def drifted(G, seed):
    """G [n, 4, 4] float64 composed with accumulated per-frame drift (<= 0.01 rad, <= 0.05 m) -> float32 [n, 16]"""
    rng = np.random.default_rng(seed)
    n = G.shape[0]
    out, D = np.empty((n, 4, 4)), np.eye(4)
    for k in range(n):
        axis = rng.normal(size=3)
        axis *= rng.uniform(0, 0.01) / np.linalg.norm(axis)
        th = np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]]) / th
        d = np.eye(4)
        d[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        step = rng.normal(size=3)
        d[:3, 3] = step * rng.uniform(0, 0.05) / np.linalg.norm(step)
        D = D @ d
        out[k] = G[k] @ D
    return out.reshape(n, 16).astype(np.float32)


def timed(ctx, ev, params, reps, warmup):
    """median, min, max milliseconds of one launch (device events)"""
    import torch
    for _ in range(warmup):
        ev.evaluate(ctx, params)
    torch.cuda.synchronize()
    events = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for e in events:
        e[0].record()
        ev.evaluate(ctx, params)
        e[1].record()
    torch.cuda.synchronize()
    times = np.array([e[0].elapsed_time(e[1]) for e in events])
    return float(np.median(times)), float(times.min()), float(times.max())


def run(ctx, B, rows, gt16, est16, host_sample, breakdown, device=0):
    import torch
    import trajectory_ref as tr
    from srrg2_proslam_amd import ops
    dev = torch.device("cuda", device)
    ev = ops.TrajectoryEvalBatch(device, B, rows, with_valid=False)
    idx = torch.arange(B, device=dev) % UNIQUE
    ev.estimate.copy_(torch.from_numpy(est16).to(dev).index_select(0, idx))
    ev.ground_truth.copy_(torch.from_numpy(gt16).to(dev).unsqueeze(0).expand(B, rows, 16))
    ev.n_frames.fill_(rows)
    params = ops.trajectory_params()
    reps, warmup = (200, 20) if B <= 256 else (20, 3)
    device_ms, device_min, device_max = timed(ctx, ev, params, reps, warmup)
    parts = {}
    if breakdown:
        variants = (("one_length", ops.trajectory_params(lengths=(100,))), ("no_kitti", ops.trajectory_params(kitti_step=0)),
                    ("no_kitti_no_alignment", ops.trajectory_params(align="none", kitti_step=0)),
                    ("no_kitti_no_alignment_no_rpe", ops.trajectory_params(align="none", kitti_step=0, rpe_delta=rows)))
        parts = {name: timed(ctx, ev, p, reps, warmup)[0] * 1e3 for name, p in variants}
        ev.evaluate(ctx, params)  # the results read below are the full metric's
    # the host route: copy the estimates out, walk them in numpy
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = ev.estimate.cpu().numpy()
    copy_s = time.perf_counter() - t0
    sample = min(host_sample, B)
    t0 = time.perf_counter()
    refs = [tr.evaluate(host[b], gt16) for b in range(sample)]
    numpy_s = (time.perf_counter() - t0) / sample
    got = ev.results()
    worst = 0.0  # the kernel against the restatement on the sampled sequences, relative to |want| + 1
    for b in range(sample):
        assert got[b]["status"] == 0 and got[b]["n_kitti"] == refs[b]["n_kitti"]
        for k in ("ate_rmse", "rpe_t_rmse", "rpe_r_rmse", "kitti_t", "kitti_r", "path_length"):
            worst = max(worst, abs(got[b][k] - refs[b][k]) / (abs(refs[b][k]) + 1.0))
    bytes_algorithmic = B * rows * 128
    return {"batch": B, "rows": rows, "device_ms": device_ms, "device_ms_min": device_min, "device_ms_max": device_max,
            "reps": reps, "breakdown_us": parts, "algorithmic_bytes": bytes_algorithmic, "achieved_GB_per_s": bytes_algorithmic / (device_ms * 1e-3) / 1e9,
            "host_copy_ms": copy_s * 1e3, "host_numpy_ms_per_sequence": numpy_s * 1e3,
            "host_route_ms_copy_plus_numpy_scaled_to_batch": copy_s * 1e3 + numpy_s * 1e3 * B, "host_sample": sample,
            "ate_rmse_m": [got[b]["ate_rmse"] for b in range(sample)], "kitti_t_percent": [100.0 * got[b]["kitti_t"] for b in range(sample)],
            "worst_relative_deviation_from_numpy": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,256,4096")
    ap.add_argument("--rows", type=int, default=4541)
    ap.add_argument("--host-sample", type=int, default=4)
    ap.add_argument("--breakdown", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_trajectory.py measures on the GPU; none is visible")
    import trajectory_ref as tr
    from srrg2_proslam_amd import ops
    G = tr.to44(np.load(os.path.join(ROOT, "tests", "golden", "ref_kitti_gt.npz"))["city"][:args.rows])
    rows = G.shape[0]
    gt16 = G.reshape(rows, 16).astype(np.float32)
    est16 = np.stack([drifted(G, 1000 + u) for u in range(UNIQUE)])
    ctx = ops.Context(0)
    runs = [run(ctx, int(b), rows, gt16, est16, args.host_sample, args.breakdown) for b in args.batches.split(",")]
    ctx.close()
    print(json.dumps({"metric": "trajectory evaluation (ATE, RPE, KITTI block) of B sequences on the device against the host route", "runs": runs}))


if __name__ == "__main__":
    main()
