#!/usr/bin/env python3
"""The world map (ops.WorldMapBatch: prs_world_map_batch_run) at three shapes -- one sequence of 443 maps of 4096 landmarks (KITTI-00
with the shipped split settings), and 256 and 4096 sequences of a few maps each -- beside the host route it replaces:
`MapArchive.slot_of` per map (a `.cpu()` per array) plus the numpy restatement's float64 transform (tests/world_map_ref.py).

Every map is full and the default parameters keep every row, so a call moves the algorithmic 53 bytes in (coords, descriptor, n_opt,
inlier) and 60 bytes out (xyz, descriptor, node, row, n_opt) per landmark; the count pass reads coords, n_opt and inlier a second time
(21 bytes), which the achieved rate does not credit.  Device time: device events around `reps` calls after a warm-up, median; a call
is up to four launches (count, scan, scatter, bounds).  The host route is timed on `--host-sample` sequences and scaled to B (it is a
per-map Python loop), and says so in its key.  The sampled sequences' clouds are compared with the host route's, byte for byte.

    python tools/bench_world_map.py [--shapes 1x443,256x4,4096x3] [--capacity 4096] [--host-sample 1]
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

HBM_MEASURED_TB_S, HBM_SPEC_TB_S = 6.29, 8.0  # a float4 copy on an MI355X, and the data sheet
BYTES_IN, BYTES_OUT, BYTES_COUNT = 53, 60, 21


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


def run(ctx, B, n_maps, capacity, host_sample, device=0):
    """B sequences of n_maps full maps: n_maps - 1 archived ones on nodes 0 .. n_maps - 2 and the live one on the last node"""
    import torch
    import world_map_cases as wc
    import world_map_ref as ref
    from srrg2_proslam_amd import ops
    dev = torch.device("cuda", device)
    S, NS = max(n_maps - 1, 1), n_maps + 1
    maps = ops.MapBatch(device, B, capacity, 0, 1, 1, 1)
    frames = ops.AlignFrames(device, B, 1, 1)
    graphs = ops.PoseGraphBatch(device, B, NS, NS, envelope_blocks=4)
    sess = ops.SessionBatch(device, maps, frames, graphs, 1)
    arch = ops.MapArchive(device, maps, NS, S)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    for holder in (maps, arch):
        holder.coords.copy_(torch.randn(holder.coords.shape, generator=gen, device=dev) * 20)
        holder.desc.copy_(torch.randint(0, 256, holder.desc.shape, generator=gen, device=dev, dtype=torch.uint8))
        holder.n_opt.copy_(torch.randint(0, 6, holder.n_opt.shape, generator=gen, device=dev, dtype=torch.int32))
        holder.inlier.copy_(torch.randint(0, 2, holder.inlier.shape, generator=gen, device=dev, dtype=torch.uint8))
        holder.n_points.fill_(capacity)
    rng = np.random.default_rng(7)
    X = np.stack([wc.rigid(rng, scale=1000.0) for _ in range(NS)])
    graphs.X.copy_(torch.from_numpy(X).to(dev).reshape(1, NS, 16).expand(B, NS, 16))
    graphs.n_nodes.fill_(n_maps)
    sess.cur_node.fill_(n_maps - 1)
    son = np.full(NS, -1, np.int32)
    son[:n_maps - 1] = np.arange(n_maps - 1)
    arch.slot_of_node.copy_(torch.from_numpy(son).to(dev).reshape(1, NS).expand(B, NS))
    rows = n_maps * capacity
    wm = ops.WorldMapBatch(sess, maps, arch, rows)
    params = ops.world_map_params()
    reps, warmup = (100, 10) if B * rows < (1 << 24) else (10, 2)
    run_ms = timed(lambda: wm.run(ctx, params), reps, warmup)
    count_ms = timed(lambda: wm.count(ctx, params), reps, warmup)
    refresh_ms = timed(lambda: wm.run(ctx, ops.world_map_params(refresh_state=True)), reps, warmup)
    wm.run(ctx, params)
    torch.cuda.synchronize()
    assert wm.status.eq(0).all().item() and wm.n_total.eq(rows).all().item()
    # the host route on the sampled sequences: slot_of per map, then numpy; compared with the device's cloud
    sample = min(host_sample, B)
    p = ref.params()
    t0 = time.perf_counter()
    clouds = []
    for b in range(sample):
        archived = [(n, arch.slot_of(b, n)) for n in range(n_maps - 1)]
        live = (n_maps - 1, dict(coords=maps.coords[b].cpu().numpy(), n_opt=maps.n_opt[b].cpu().numpy(), inlier=maps.inlier[b].cpu().numpy(),
                                 n_points=int(maps.n_points[b].item())))
        clouds.append(ref.host_route(archived, live, X, p))
    host_s = (time.perf_counter() - t0) / sample
    for b in range(sample):
        assert wm.cloud_of(b)["xyz"].tobytes() == clouds[b].tobytes(), "device cloud differs from the host route's"
    total = B * rows
    moved = total * (BYTES_IN + BYTES_OUT)
    rate = moved / (run_ms[0] * 1e-3) / 1e12
    return {"batch": B, "maps": n_maps, "capacity": capacity, "landmarks": total, "reps": reps,
            "run_ms": run_ms[0], "run_ms_min": run_ms[1], "run_ms_max": run_ms[2],
            "count_ms": count_ms[0], "count_ms_min": count_ms[1], "count_ms_max": count_ms[2],
            "run_with_refresh_state_ms": refresh_ms[0],
            "algorithmic_bytes": moved, "achieved_TB_per_s": rate, "of_hbm_measured_copy_rate": rate / HBM_MEASURED_TB_S,
            "of_hbm_spec": rate / HBM_SPEC_TB_S, "count_achieved_TB_per_s": total * BYTES_COUNT / (count_ms[0] * 1e-3) / 1e12,
            "ns_per_landmark": run_ms[0] * 1e6 / total,
            "host_route_ms_per_sequence": host_s * 1e3, "host_route_ms_scaled_to_batch": host_s * 1e3 * B, "host_sample": sample,
            "clouds_equal_host_route": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x443,256x4,4096x3", help="BxMAPS, comma separated")
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--host-sample", type=int, default=1)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_world_map.py measures on the GPU; none is visible")
    from srrg2_proslam_amd import ops
    ctx = ops.Context(0)
    runs = []
    for shape in args.shapes.split(","):
        B, n_maps = (int(v) for v in shape.split("x"))
        runs.append(run(ctx, B, n_maps, args.capacity, args.host_sample))
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps({"metric": "world map (landmark cloud of B sequences from archive, live map and graph) on the device against the host route",
                      "hbm_TB_per_s": {"measured_copy": HBM_MEASURED_TB_S, "spec": HBM_SPEC_TB_S}, "runs": runs}))


if __name__ == "__main__":
    main()
