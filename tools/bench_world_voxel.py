#!/usr/bin/env python3
"""The world voxel filter (ops.WorldVoxelBatch: prs_world_voxel_batch_run) at the world-map bench's three shapes -- one sequence of
443 maps of 4096 landmarks (KITTI-00 with the shipped split settings), and 256 and 4096 sequences of a few maps each -- beside the
host route the parent offers: a cloud copied to the host as `WorldMapBatch.cloud_of` copies it (one `.cpu()` per array) plus a numpy
voxel filter (tests/world_voxel_ref.py: keys, a sort, the representative per voxel).

The clouds are seeded, uniformly random in a cube, full (in_n = in_stride), in the layout the world map writes.  The voxel size sets
the share of rows that survive: n rows over V equally likely voxels leave V * (1 - exp(-n / V)) of them, so V = 1000 n, n / 1.594 and
n / 10 leave roughly all, a half and a tenth.  A real cloud's repeats sit in clusters (the same corner seen from consecutive maps),
which a uniform cloud does not imitate: its equal keys are spread over the whole input.  Device time: device events around `reps`
calls after a warm-up, median; a call is five launches (clear, insert, flag, scan, scatter), the table has the default 2 x in_stride
slots rounded up to a power of two.  The sampled sequences' representatives are compared with the host route's.

    python tools/bench_world_voxel.py [--shapes 1x443,256x4,4096x3] [--capacity 4096] [--host-sample 1] [--breakdown]
prints one JSON line.  --breakdown adds the per-kernel split: every (shape, share, position) runs once more in a child process of its
own under `rocprofv3 --kernel-trace --stats`, profiler off for the event times.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EDGE = 200.0  # metres, the cube the rows lie in
SHARES = {"all": 1000.0, "half": 1.0 / 1.594, "tenth": 0.1}  # voxels per row
# per input row: the insert reads xyz and n_opt and writes the row's slot; flag and scatter read the slot back.  Per voxel written:
# xyz, descriptor, node, row, n_opt in and out, index and count out.  Per table slot: 48 bytes cleared
BYTES_ROW, BYTES_VOXEL, BYTES_SLOT = 16 + 4 + 4 + 4 + 4, 2 * 64 + 8, 48


def timed(fn, reps, warmup):
    """median, min, max milliseconds of one call (device events)"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    events = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for e in events:
        e[0].record()
        fn()
        e[1].record()
    torch.cuda.synchronize()
    times = np.array([e[0].elapsed_time(e[1]) for e in events])
    return float(np.median(times)), float(times.min()), float(times.max())


def voxel_size(rows, share):
    return EDGE / (rows * SHARES[share]) ** (1.0 / 3.0)


def make_cloud(B, rows, capacity, device=0):
    import torch
    dev = torch.device("cuda", device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    xyz = (torch.rand((B, rows, 4), generator=gen, device=dev) - 0.5) * EDGE
    i = torch.arange(rows, device=dev, dtype=torch.int32).reshape(1, rows).expand(B, rows).contiguous()
    return dict(xyz=xyz, n_out=torch.full((B,), rows, dtype=torch.int32, device=dev),
                n_opt=torch.randint(0, 6, (B, rows), generator=gen, device=dev, dtype=torch.int32),
                desc=torch.randint(0, 256, (B, rows, 32), generator=gen, device=dev, dtype=torch.uint8),
                node=torch.div(i, capacity, rounding_mode="floor").to(torch.int32), row=i % capacity)


def run(ctx, B, n_maps, capacity, shares, positions, host_sample, reps_override=None):
    import torch
    import world_voxel_ref as ref
    from srrg2_proslam_amd import ops
    rows = n_maps * capacity
    cloud = make_cloud(B, rows, capacity)
    vx = ops.WorldVoxelBatch(B, rows, rows)
    reps, warmup = (100, 10) if B * rows < (1 << 24) else (10, 2)
    if reps_override:
        reps, warmup = reps_override, 2
    out = {"batch": B, "maps": n_maps, "capacity": capacity, "rows": B * rows, "table_stride": vx.table_stride, "reps": reps,
           "workspace_bytes": int(vx.workspace.numel()), "cases": []}
    for share in shares:
        s = voxel_size(rows, share)
        case = {"share": share, "voxel_size": s}
        for position in positions:
            p = ops.world_voxel_params(s, position)
            ms = timed(lambda: vx.run(ctx, p, cloud), reps, warmup)
            count_ms = timed(lambda: vx.count(ctx, p, cloud), reps, warmup)
            torch.cuda.synchronize()
            assert vx.status.eq(0).all().item() and vx.n_nonfinite.eq(0).all().item() and vx.n_outside.eq(0).all().item()
            voxels = int(vx.n_voxels.sum().item())
            atomics = 3 + (3 if position == "mean" else 0)  # compare-and-swap (first probe), min, add; MEAN: three more adds
            moved = B * rows * BYTES_ROW + voxels * BYTES_VOXEL + B * vx.table_stride * BYTES_SLOT
            case[position] = {"run_ms": ms[0], "run_ms_min": ms[1], "run_ms_max": ms[2], "count_ms": count_ms[0],
                              "voxels": voxels, "share_kept": voxels / (B * rows), "atomics_per_row": atomics,
                              "atomic_bytes_per_row": 8 + 8 + 4 + (24 if position == "mean" else 0),
                              "algorithmic_bytes": moved, "achieved_TB_per_s": moved / (ms[0] * 1e-3) / 1e12,
                              "ns_per_row": ms[0] * 1e6 / (B * rows)}
        if host_sample:
            # the host route on the sampled sequences: the copies cloud_of makes, then numpy; compared with the device's representatives
            p = ops.world_voxel_params(s, "representative")
            vx.run(ctx, p, cloud)
            torch.cuda.synchronize()
            sample = min(host_sample, B)
            t0 = time.perf_counter()
            index = []
            for b in range(sample):
                host = {k: cloud[k][b, :rows].cpu().numpy().copy() for k in ("xyz", "desc", "node", "row", "n_opt")}
                index.append(ref.host_route(host["xyz"], host["n_opt"], s))
            host_s = (time.perf_counter() - t0) / sample
            for b in range(sample):
                assert vx.cloud_of(b)["index"].tolist() == index[b].tolist(), "device representatives differ from the host route's"
            case.update(host_route_ms_per_sequence=host_s * 1e3, host_route_ms_scaled_to_batch=host_s * 1e3 * B, host_sample=sample,
                        representatives_equal_host_route=True)
        out["cases"].append(case)
    return out


def breakdown(shape, capacity, share, position):
    """the per-kernel split of one configuration: this tool again, in a child process under the profiler -> {kernel: microseconds}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--shapes", shape, "--capacity", str(capacity), "--shares", share, "--positions", position, "--host-sample", "0", "--reps", "20"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        split = {}
        for f in glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                name = r["Name"]
                if "world_voxel_" in name:
                    short = name[name.index("world_voxel_"):].split("(")[0].split("ENS")[0]
                    split[short] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                                    "max_us": float(r["MaxNs"]) / 1e3}
        return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x443,256x4,4096x3", help="BxMAPS, comma separated")
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--shares", default="all,half,tenth")
    ap.add_argument("--positions", default="representative,mean")
    ap.add_argument("--host-sample", type=int, default=1)
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--breakdown", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_world_voxel.py measures on the GPU; none is visible")
    from srrg2_proslam_amd import ops
    shares, positions = args.shares.split(","), args.positions.split(",")
    ctx = ops.Context(0)
    runs = []
    for shape in args.shapes.split(","):
        B, n_maps = (int(v) for v in shape.split("x"))
        runs.append(run(ctx, B, n_maps, args.capacity, shares, positions, args.host_sample, args.reps))
        torch.cuda.empty_cache()
    ctx.close()
    if args.breakdown:  # the children open the device after this process has let go of its tensors
        for shape, r in zip(args.shapes.split(","), runs):
            for case in r["cases"]:
                for position in positions:
                    case[position]["kernels"] = breakdown(shape, args.capacity, case["share"], position)
    print(json.dumps({"metric": "world voxel filter (one row per voxel of B world clouds) on the device against cloud_of plus numpy",
                      "runs": runs}))


if __name__ == "__main__":
    main()
