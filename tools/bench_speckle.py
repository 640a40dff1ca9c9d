"""Speckle filter throughput (prs_speckle_batch_run): B disparity or depth images resident in HBM, filtered in place.
usage: python tools/bench_speckle.py [kitti|euroc|vga ...] [--batch N ...] [--input NAME ...] [--max-size N] [--max-diff X] [--rounds N]
                                     [--json FILE] [--breakdown-batch N] [--no-breakdown] [--no-check] [--once]
  Shapes: kitti 376 x 1241 and euroc 480 x 752, float32 disparity; vga 640 x 480, 16-bit depth in millimetres.  Batches default to
  1 64 1024 (a batch that does not fit the free memory is skipped).  Inputs, four distinct images replicated over the batch:
    stereo      the disparity of a DenseStereoBatch run on a seeded textured pair whose disparity changes from band to band of 47
                rows, the last eight rows of a band unrelated in the two images and 15 % of the left pixels redrawn, so that the
                matcher leaves islands (vga: its depth, in millimetres): the typical case
    one         a constant image: one component, every add of a size to one word
    serpentine  every other row whole, joined at alternating ends: one path through every tile and across every seam, the longest walks
  The first and the last image of every configuration are compared with the restatement (tests/speckle_ref.py) byte for byte before anything is
  timed.  The call works in place, so every timed call is preceded by an untimed copy that restores the image; each call has its own
  pair of events on the stream; the inputs take turns round by round (median and minimum over the rounds):
    call          ms per call (tile, seam, flatten, apply) and us per image
    copy          a device-to-device copy of the floor's bytes
    dense stereo  the prs_dense_stereo_batch_run call that produces the disparity, on the same shape and batch (128 disparities)
  floor: the bytes the four launches cannot avoid -- per pixel the image read (4 or 2), the parents written by the tile launch (4)
  and read by flatten and by apply (8), the sizes zeroed (4): 20 or 18; the seam launch's reads, the parents flatten rewrites, the
  sizes read at the roots and the zeroes written are not in it -- at the bandwidth the copy reached.
  --breakdown (default, at --breakdown-batch): the configuration once more in a child process of its own under
  `rocprofv3 --kernel-trace --stats`, for the time per kernel.  --once: five calls and no timing (what the child runs)."""
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

VGA = {"fx": 525.0, "fy": 525.0, "cx": 319.5, "cy": 239.5, "baseline_m": 0.075}  # a structured-light sensor's geometry
SHAPES = {"kitti": (376, 1241, configs.KITTI["camera"], "f32"), "euroc": (480, 752, configs.EUROC["camera"], "f32"), "vga": (480, 640, VGA, "u16")}
INPUTS = ("stereo", "one", "serpentine")
N_DISTINCT = 4


def seeded_pairs(rows, cols, n=N_DISTINCT):
    rng = np.random.default_rng(3)
    right = rng.integers(0, 256, (n, rows, cols), dtype=np.uint8)
    left = np.empty_like(right)
    xs = np.arange(cols)
    for v0 in range(0, rows, 47):
        d = 5 + (v0 * 7) % 96
        left[:, v0:v0 + 47] = right[:, v0:v0 + 47][:, :, np.clip(xs - d, 0, cols - 1)]
        left[:, v0 + 39:v0 + 47] = rng.integers(0, 256, left[:, v0 + 39:v0 + 47].shape, dtype=np.uint8)  # nothing to match: islands
    redraw = rng.random(left.shape) < 0.15
    left[redraw] = rng.integers(0, 256, int(redraw.sum()), dtype=np.uint8)
    return left, right


def serpentine(rows, cols):
    m = np.zeros((rows, cols), bool)
    m[0::2, :] = True
    m[1::4, cols - 1] = True
    m[3::4, 0] = True
    return m


def timed(fns, restore, rounds, seconds=0.2):
    """{name: (median ms, min ms)} of every fn; each call between its own two events, behind an untimed restore(name)"""
    def window(name, fn, iters):
        events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in events:
            restore(name)
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in events) / iters

    iters, times = {}, {k: [] for k in fns}
    for k, f in fns.items():
        window(k, f, 2)
        iters[k] = int(min(max(seconds * 1e3 / max(window(k, f, 2), 1e-3), 3), 200))
    for _ in range(rounds):
        for k, f in fns.items():
            times[k].append(window(k, f, iters[k]))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in times.items()}


def bench(ctx, name, B, args):
    import speckle_ref as ref
    rows, cols, camera, kind = SHAPES[name]
    dev = torch.device("cuda", 0)
    pixels = B * rows * cols
    es = 4 if kind == "f32" else 2
    floor_bytes = pixels * (es + 16)
    need = pixels * (36 + 3 * 4 + 8 + 2 * es) + floor_bytes
    free = torch.cuda.mem_get_info()[0]
    if need > 0.8 * free or pixels > 2 ** 31 - 1:
        return {"shape": name, "batch": B, "skipped": "needs %.1f GB, %.1f GB free" % (need / 1e9, free / 1e9)}
    pick = torch.arange(B, device=dev) % N_DISTINCT
    out = {"shape": name, "rows": rows, "cols": cols, "batch": B, "pixel_type": kind, "max_size": args.max_size, "max_diff": args.max_diff,
           "floor_bytes": floor_bytes}
    # the dense-stereo call in front of the filter, and its disparity as the typical input
    left_np, right_np = seeded_pairs(rows, cols)
    left = torch.from_numpy(left_np).to(dev)[pick].view(B, 1, rows, cols)
    right = torch.from_numpy(right_np).to(dev)[pick].view(B, 1, rows, cols)
    ds = ops.DenseStereoBatch(B, 1, rows, cols, outputs=("disparity", "depth"))
    dp = ops.dense_stereo_params(camera, n_disparities=128)
    stereo = lambda: ds.run(ctx, dp, left, right)  # noqa: E731
    stereo()
    torch.cuda.synchronize()
    dtype = torch.float32 if kind == "f32" else torch.uint16
    pristine = {}
    if kind == "f32":
        pristine["stereo"] = ds.disparity.contiguous()
    else:  # millimetres, as a sensor delivers them; what lies beyond 16 bits is no measurement
        mm = torch.round(ds.depth * 1000.0)
        pristine["stereo"] = torch.where(mm < 65536.0, mm, torch.zeros_like(mm)).to(torch.int32).to(dtype).contiguous()
    pristine["one"] = torch.full((B, 1, rows, cols), 7, dtype=torch.int32, device=dev).to(dtype)
    snake = torch.from_numpy(serpentine(rows, cols).astype(np.int32) * 7).to(dev)
    pristine["serpentine"] = snake.view(1, 1, rows, cols).expand(B, 1, rows, cols).to(dtype).contiguous()
    pristine = {k: v for k, v in pristine.items() if k in args.input}
    image = torch.empty((B, 1, rows, cols), dtype=dtype, device=dev)
    sf = ops.SpeckleFilterBatch(B, 1, rows, cols)
    p = ops.speckle_params(args.max_size, args.max_diff, pixel_type=kind)
    out["workspace_bytes"] = int(sf.workspace.numel())
    run = lambda: sf.run(ctx, p, image)  # noqa: E731
    out["inputs"] = {}
    for k, src in pristine.items():
        image.copy_(src)
        run()
        torch.cuda.synchronize()
        assert int(sf.status.abs().max().item()) == 0
        kept, removed = int(sf.n_kept.sum().item()), int(sf.n_removed.sum().item())
        out["inputs"][k] = {"valid_share": (kept + removed) / pixels, "removed_share_of_valid": removed / max(kept + removed, 1)}
        if not args.no_check:
            for b in sorted({0, B - 1}):  # the first image, and the last one: the one at the highest address
                want = ref.speckle_image(src[b, 0].cpu().numpy(), None, ref.params(args.max_size, args.max_diff))
                assert image[b, 0].cpu().numpy().tobytes() == want["image"].tobytes(), "the kernels and the restatement disagree"
                assert (int(sf.n_kept[b, 0].item()), int(sf.n_removed[b, 0].item())) == (want["n_kept"], want["n_removed"])
            out["inputs"][k]["checked"] = True
    if args.once:
        for k, src in pristine.items():
            for _ in range(5):
                image.copy_(src)
                run()
        torch.cuda.synchronize()
        return out
    half = torch.empty((floor_bytes // 2 + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    other = torch.empty_like(half)
    fns = {k: run for k in pristine}
    fns["copy"] = lambda: other.copy_(half)
    fns["dense_stereo"] = stereo
    restore = lambda k: image.copy_(pristine[k]) if k in pristine else None  # noqa: E731
    t = timed(fns, restore, args.rounds)
    for k, (med, low) in t.items():
        entry = {"ms_median": med, "ms_min": low, "us_per_image": med * 1e3 / B}
        if k in pristine:
            entry["share_of_dense_stereo"] = med / t["dense_stereo"][0]
            entry["times_copy_floor"] = med / t["copy"][0]
            out["inputs"][k].update(entry)
        else:
            out[k] = entry
    out["copy_GB_per_s"] = floor_bytes / (t["copy"][0] * 1e-3) / 1e9
    return out


def breakdown(name, B, kind, args):
    """the per-kernel split of one configuration and input: this tool again, in a child process under the profiler
    -> {kernel: microseconds}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), name,
               "--batch", str(B), "--input", kind, "--max-size", str(args.max_size), "--max-diff", str(args.max_diff), "--once", "--no-check",
               "--no-breakdown"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        split = {}
        for f in glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                n = r["Name"]
                if "speckle_" in n and "_kernel" in n:
                    short = n[n.index("speckle_") + 8:n.index("_kernel")]
                    split[short] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3}
        return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", default=list(SHAPES))
    ap.add_argument("--batch", nargs="*", type=int, default=[1, 64, 1024])
    ap.add_argument("--input", nargs="*", default=list(INPUTS), choices=INPUTS)
    ap.add_argument("--max-size", type=int, default=configs.SPECKLE["max_size"])
    ap.add_argument("--max-diff", type=float, default=configs.SPECKLE["max_diff"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--breakdown-batch", type=int, default=64)
    ap.add_argument("--no-breakdown", action="store_true")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_speckle.py measures on the GPU"
    ctx = ops.Context(0)
    results = []
    for name in args.shape:
        for B in args.batch:
            r = bench(ctx, name, B, args)
            results.append(r)
            torch.cuda.empty_cache()
            if "skipped" in r:
                print("%s x %d: skipped (%s)" % (name, B, r["skipped"]), flush=True)
                continue
            print("%s %d x %d %s, B = %d, max_size %d, max_diff %g (workspace %.1f MB)" % (
                name, r["rows"], r["cols"], r["pixel_type"], B, args.max_size, args.max_diff, r["workspace_bytes"] / 1e6), flush=True)
            if "copy" in r:
                print("  dense stereo %.3f ms; copy of the floor's %.1f MB %.3f ms (%.0f GB/s)" % (
                    r["dense_stereo"]["ms_median"], r["floor_bytes"] / 1e6, r["copy"]["ms_median"], r["copy_GB_per_s"]), flush=True)
            for k, v in r["inputs"].items():
                line = "  %-10s %.0f %% valid, %.1f %% of them removed" % (k, 100 * v["valid_share"], 100 * v["removed_share_of_valid"])
                if "ms_median" in v:
                    line += ": call %.3f ms (min %.3f), %.1f us an image, %.1f %% of the dense-stereo call, %.1f times the copy" % (
                        v["ms_median"], v["ms_min"], v["us_per_image"], 100 * v["share_of_dense_stereo"], v["times_copy_floor"])
                print(line, flush=True)
    ctx.close()
    if not args.no_breakdown and not args.once:  # the children open the device after this process has let go of its tensors
        for r in results:
            if "skipped" in r or r["batch"] != args.breakdown_batch:
                continue
            for k in r["inputs"]:
                try:
                    split = breakdown(r["shape"], r["batch"], k, args)
                except (subprocess.SubprocessError, OSError) as e:
                    print("%s B = %d %s per kernel: the profiler run failed (%s)" % (r["shape"], r["batch"], k, e), flush=True)
                    continue
                r["inputs"][k]["kernels"] = split
                print("%s B = %d %s per kernel: %s" % (r["shape"], r["batch"], k, ", ".join(
                    "%s %.1f us" % (n, v["average_us"]) for n, v in sorted(split.items()))), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
