"""Depth consistency filter throughput (prs_depth_consistency_batch_run): B sequences of depth frames resident in HBM, filtered into out.
usage: python tools/bench_depth_consistency.py [vga|kitti ...] [--layout BxF ...] [--window N ...] [--rounds N] [--json FILE]
                                               [--breakdown-layout BxF] [--no-breakdown] [--no-check] [--no-counts] [--once]
  Shapes: vga 640 x 480, 16-bit depth in millimetres; kitti 376 x 1241, float32 depth in metres.  Layouts default to 1x64 64x16 256x4
  (sequences x frames; one that does not fit the free memory is skipped), windows to 1 2 4.  Input: the scene of
  tests/depth_consistency_ref.py -- a wall 5 m away with a rectangle 3 m away in front of it -- seen from `frames` cameras 3 cm and 4
  mrad apart, 5 % of the pixels' depths off by a factor; every sequence of the batch holds a copy of its own.  Where the whole
  restatement is affordable (frames * 2 * window <= 32) the first and the last sequence are compared with it byte for byte before anything is timed.
  Each call has its own pair of events on the stream; the calls take turns round by round (median and minimum over the rounds):
    call         ms per call (prepare, filter) and us per image
    copy         a device-to-device copy of the floor's bytes
    dense cloud  the prs_depth_cloud_batch_run call on the same images, the stage the filter stands in front of
  floor: per pixel the image read once for itself and once for every existing slot -- the gathers of a tile touch a patch of the
  neighbour of the tile's size -- and out written once: (1 + slots) reads and one write of the element, slots averaged over the
  frames of a sequence, at the bandwidth the copy reached.
  --breakdown (default, at --breakdown-layout): the configuration once more in a child process of its own under
  `rocprofv3 --kernel-trace --stats`, for the time per kernel.  --once: five calls and no timing (what the child runs).
  --no-counts: the call without n_kept / n_removed, so without its atomic adds."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from srrg2_proslam_amd import configs, ops  # noqa: E402

VGA = {"fx": 525.0, "fy": 525.0, "cx": 319.5, "cy": 239.5}  # a structured-light sensor's geometry
SHAPES = {"vga": (480, 640, VGA, "u16", 1e-3), "kitti": (376, 1241, configs.KITTI["camera"], "f32", 1.0)}


def sequence(rows, cols, camera, kind, frames):
    """(depth [frames, rows, cols], pose [frames, 16]) on the host"""
    import depth_consistency_ref as ref
    rng = np.random.default_rng(5)
    mid = (frames - 1) / 2
    pose = np.stack([ref.yaw_pose(0.004 * (i - mid), (0.03 * (i - mid), 0.002 * i, 0.01 * i)) for i in range(frames)])
    depth = np.stack([ref.scene_depth(T, rows, cols, camera) for T in pose])
    planted = rng.random(depth.shape) < 0.05
    factor = np.where(rng.random(depth.shape) < 0.5, rng.uniform(0.5, 0.8, depth.shape), rng.uniform(1.25, 2.0, depth.shape))
    depth = np.where(planted, depth * factor, depth).astype(np.float32)
    return (np.round(depth * 1000).astype(np.uint16) if kind == "u16" else depth), pose


def timed(fns, rounds, seconds=0.2):
    """{name: (median ms, min ms)} of every fn; each call between its own two events"""
    def window(fn, iters):
        events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in events:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in events) / iters

    iters, times = {}, {k: [] for k in fns}
    for k, f in fns.items():
        window(f, 2)
        iters[k] = int(min(max(seconds * 1e3 / max(window(f, 2), 1e-3), 3), 200))
    for _ in range(rounds):
        for k, f in fns.items():
            times[k].append(window(f, iters[k]))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in times.items()}


def mean_slots(frames, window):
    return sum(sum(0 <= g < frames for j in range(1, window + 1) for g in (f - j, f + j)) for f in range(frames)) / frames


def bench(ctx, name, B, frames, args):
    import depth_consistency_ref as ref
    rows, cols, camera, kind, scale = SHAPES[name]
    dev = torch.device("cuda", 0)
    pixels = B * frames * rows * cols
    es = 4 if kind == "f32" else 2
    worst_floor = pixels * es * (2 + 2 * max(args.window))
    need = pixels * (2 * es + 16 + 8) + worst_floor
    free = torch.cuda.mem_get_info()[0]
    label = "%dx%d" % (B, frames)
    if need > 0.8 * free or pixels > 2 ** 31 - 1:
        return {"shape": name, "layout": label, "skipped": "needs %.1f GB, %.1f GB free" % (need / 1e9, free / 1e9)}
    out = {"shape": name, "rows": rows, "cols": cols, "layout": label, "batch": B, "frames": frames, "depth_type": kind, "windows": {}}
    depth_np, pose_np = sequence(rows, cols, camera, kind, frames)
    depth = torch.from_numpy(depth_np).to(dev).unsqueeze(0).expand(B, frames, rows, cols).contiguous()
    pose = torch.from_numpy(pose_np).to(dev).unsqueeze(0).expand(B, frames, 16).contiguous()
    dcb = ops.DepthConsistencyBatch(B, frames, rows, cols, max(args.window), kind, outputs=() if args.no_counts else ("n_kept", "n_removed"))
    kw = dict(configs.DEPTH_CONSISTENCY)
    params = {w: ops.depth_consistency_params(camera, **dict(kw, window=w), depth_type=kind, scale=scale) for w in args.window}
    runs = {w: (lambda w=w: dcb.run(ctx, params[w], depth, pose)) for w in args.window}
    for w in args.window:
        runs[w]()
        torch.cuda.synchronize()
        assert int(dcb.status.abs().max().item()) == 0
        entry = {"slots": mean_slots(frames, w)}
        if not args.no_counts:
            kept, removed = int(dcb.n_kept.sum().item()), int(dcb.n_removed.sum().item())
            entry.update(valid_share=(kept + removed) / pixels, removed_share_of_valid=removed / max(kept + removed, 1))
        entry["floor_bytes"] = int(pixels * es * (2 + entry["slots"]))
        if not args.no_check and frames * 2 * w <= 32:
            want = ref.depth_consistency(dict(depth=depth_np, pose=pose_np), ref.params(camera, **dict(kw, window=w), scale=scale))
            for b in sorted({0, B - 1}):
                got = dcb.out[b].cpu().numpy()
                assert all(got[f].tobytes() == r["out"].tobytes() for f, r in enumerate(want["results"])), "the kernels and the restatement disagree"
                assert args.no_counts or dcb.n_kept[b].cpu().tolist() == [r["n_kept"] for r in want["results"]]
            entry["checked"] = True
        out["windows"][w] = entry
    if args.once:
        for w in args.window:
            for _ in range(5):
                runs[w]()
        torch.cuda.synchronize()
        return out
    dc = ops.DepthCloudBatch(B, frames, rows, cols, frames * rows * cols)
    cp = ops.depth_cloud_params(camera, kw["range_min"], kw["range_max"], 1, kind, scale)
    n_images = torch.full((B,), frames, dtype=torch.int32, device=dev)
    fns = {"window %d" % w: runs[w] for w in args.window}
    fns["dense_cloud"] = lambda: dc.run(ctx, cp, depth, pose, n_images)
    halves = {}
    for w in args.window:
        half = torch.empty((out["windows"][w]["floor_bytes"] // 2 + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        halves[w] = (half, torch.empty_like(half))
        fns["copy %d" % w] = lambda w=w: halves[w][1].copy_(halves[w][0])
    t = timed(fns, args.rounds)
    images = B * frames
    out["dense_cloud"] = {"ms_median": t["dense_cloud"][0], "ms_min": t["dense_cloud"][1], "us_per_image": t["dense_cloud"][0] * 1e3 / images}
    for w in args.window:
        med, low = t["window %d" % w]
        copy = t["copy %d" % w][0]
        out["windows"][w].update(ms_median=med, ms_min=low, us_per_image=med * 1e3 / images, copy_ms=copy,
                                 copy_GB_per_s=out["windows"][w]["floor_bytes"] / (copy * 1e-3) / 1e9, times_copy_floor=med / copy,
                                 times_dense_cloud=med / t["dense_cloud"][0])
    return out


def breakdown(name, layout, window):
    """the per-kernel split of one configuration: this tool again, in a child process under the profiler -> {kernel: microseconds}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), name,
               "--layout", layout, "--window", str(window), "--once", "--no-check", "--no-breakdown"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        split = {}
        for f in glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                n = r["Name"]
                if "depth_consistency_" in n and "_kernel" in n:
                    short = n[n.index("depth_consistency_") + 18:n.index("_kernel")]
                    split[short] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3}
        return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", default=list(SHAPES))
    ap.add_argument("--layout", nargs="*", default=["1x64", "64x16", "256x4"])
    ap.add_argument("--window", nargs="*", type=int, default=[1, 2, 4])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--breakdown-layout", default="64x16")
    ap.add_argument("--no-breakdown", action="store_true")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-counts", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_consistency.py measures on the GPU"
    ctx = ops.Context(0)
    results = []
    for name in args.shape:
        for layout in args.layout:
            B, frames = (int(x) for x in layout.split("x"))
            r = bench(ctx, name, B, frames, args)
            results.append(r)
            torch.cuda.empty_cache()
            if "skipped" in r:
                print("%s %s: skipped (%s)" % (name, layout, r["skipped"]), flush=True)
                continue
            print("%s %d x %d %s, %d sequences of %d frames" % (name, r["rows"], r["cols"], r["depth_type"], B, frames), flush=True)
            if "dense_cloud" in r:
                print("  dense cloud %.3f ms, %.2f us an image" % (r["dense_cloud"]["ms_median"], r["dense_cloud"]["us_per_image"]), flush=True)
            for w, v in r["windows"].items():
                line = "  window %d (%.2f slots a frame)" % (w, v["slots"])
                if "valid_share" in v:
                    line += " %.0f %% valid, %.1f %% of them removed" % (100 * v["valid_share"], 100 * v["removed_share_of_valid"])
                line += ", checked" if v.get("checked") else ""
                if "ms_median" in v:
                    line += ": call %.3f ms (min %.3f), %.2f us an image; copy of %.1f MB %.3f ms (%.0f GB/s): %.2f times the copy, %.2f times the dense cloud" % (
                        v["ms_median"], v["ms_min"], v["us_per_image"], v["floor_bytes"] / 1e6, v["copy_ms"], v["copy_GB_per_s"],
                        v["times_copy_floor"], v["times_dense_cloud"])
                print(line, flush=True)
    ctx.close()
    if not args.no_breakdown and not args.once:  # the children open the device after this process has let go of its tensors
        for r in results:
            if "skipped" in r or r["layout"] != args.breakdown_layout:
                continue
            for w in r["windows"]:
                try:
                    split = breakdown(r["shape"], r["layout"], w)
                except (subprocess.SubprocessError, OSError) as e:
                    print("%s %s window %d per kernel: the profiler run failed (%s)" % (r["shape"], r["layout"], w, e), flush=True)
                    continue
                r["windows"][w]["kernels"] = split
                print("%s %s window %d per kernel: %s" % (r["shape"], r["layout"], w, ", ".join(
                    "%s %.1f us" % (n, v["average_us"]) for n, v in sorted(split.items()))), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
