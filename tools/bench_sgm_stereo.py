"""Semi-global dense stereo throughput (prs_sgm_stereo_batch_run): B rectified pairs resident in HBM to disparity and depth images.
usage: python tools/bench_sgm_stereo.py [kitti|euroc ...] [--batch N ...] [--paths N ...] [--disparities N] [--in-flight N] [--rounds N]
                                        [--json FILE] [--no-breakdown] [--no-check] [--once]
  Shapes: kitti 376 x 1241, euroc 480 x 752; batches default to 1 64 1024 (a batch that does not fit the free memory is skipped),
  paths to 4 and 8.  The pairs are those of tools/bench_dense_stereo.py: four distinct right images of random bytes, the left ones
  shifted by a disparity that changes from band to band of rows, replicated over the batch.  The first and the last pair are compared with the
  restatement (tests/sgm_stereo_ref.py) byte for byte before anything is timed.
  Per shape, batch and path count, timed with events on the stream in interleaved rounds (median and minimum over the rounds):
    call       ms per call (census, per chunk of images_in_flight images a path launch a direction, a winner and a right-winner
               launch, finish) and
               us per pair; images_in_flight is the one ops.SgmStereoBatch picks unless --in-flight gives one
    local      the prs_dense_stereo_batch_run call (radius 3) on the same pairs, in the same process
    copy       a device-to-device copy of 1 GiB, for the bandwidth of the floor
  and against them the floor:
    hbm        the bytes of S the path launches must move -- the first direction stores 2 bytes a pixel and disparity, every later
               one loads and stores them: 2 * 2 * n_paths - 2 -- at the bandwidth the copy reached.  The census words the path
               kernels read again every step (8 bytes a pixel and disparity a direction, from the caches) are not in it
  --breakdown (default): the configuration once more in a child process of its own under `rocprofv3 --kernel-trace --stats`, for
  the time per kernel, the path kernel by direction (from the order of its launches).  --once: three calls and no timing (what the
  child runs)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_dense_stereo import SHAPES, seeded_pairs  # noqa: E402
from srrg2_proslam_amd import ops  # noqa: E402

DIRECTIONS = ("(0,+1)", "(0,-1)", "(+1,0)", "(-1,0)", "(+1,+1)", "(+1,-1)", "(-1,+1)", "(-1,-1)")
COPY_BYTES = 1 << 30
ONCE_CALLS = 3
_reference = {}


def _window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _iters(fn, seconds=0.25):
    """calls in a window of at least `seconds`: one where a single call takes that long"""
    fn()
    torch.cuda.synchronize()
    return int(min(max(seconds * 1e3 / max(_window(fn, 1), 1e-3), 1), 1000))


def interleaved(fns, rounds):
    """{name: (median ms, min ms)} of every fn, timed round by round in turn"""
    iters = {k: _iters(f) for k, f in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            times[k].append(_window(f, iters[k]))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in times.items()}


def reference(name, n_paths, index, left, right, bf, n_disparities):
    import sgm_stereo_ref as ref
    key = (name, n_paths, n_disparities, index)
    if key not in _reference:
        _reference[key] = ref.sgm_stereo_image(left, right, ref.params(bf, n_disparities, 0, 10, 120, n_paths, 10, 1))
    return _reference[key]


def bench(ctx, name, B, n_paths, args):
    rows, cols, camera = SHAPES[name]
    dev = torch.device("cuda", 0)
    pixels = B * rows * cols
    in_flight = args.in_flight or ops.sgm_stereo_images_in_flight(B, 1, rows, cols, args.disparities)
    need = pixels * (2 + 2 * (8 + 26)) + 2 * min(in_flight, B) * rows * cols * args.disparities + 2 * COPY_BYTES
    free = torch.cuda.mem_get_info()[0]
    if need > 0.8 * free or pixels > 2 ** 31 - 1:
        return {"shape": name, "batch": B, "n_paths": n_paths, "skipped": "needs %.1f GB, %.1f GB free" % (need / 1e9, free / 1e9)}
    left_np, right_np = seeded_pairs(rows, cols)
    pick = torch.arange(B, device=dev) % left_np.shape[0]
    left = torch.from_numpy(left_np).to(dev)[pick].view(B, 1, rows, cols)
    right = torch.from_numpy(right_np).to(dev)[pick].view(B, 1, rows, cols)
    sg = ops.SgmStereoBatch(B, 1, rows, cols, images_in_flight=in_flight, n_disparities=args.disparities)
    p = ops.sgm_stereo_params(camera, n_disparities=args.disparities, n_paths=n_paths)
    run = lambda: sg.run(ctx, p, left, right)  # noqa: E731
    run()
    torch.cuda.synchronize()
    assert int(sg.status.abs().max().item()) == 0
    chunks = -(-B // sg.images_in_flight)
    out = {"shape": name, "rows": rows, "cols": cols, "batch": B, "n_disparities": args.disparities, "n_paths": n_paths,
           "images_in_flight": sg.images_in_flight, "launches": 2 + chunks * (n_paths + 2),
           "valid_share": float(sg.n_valid.sum().item()) / pixels, "workspace_bytes": int(sg.workspace.numel()),
           "hbm_bytes": pixels * args.disparities * (2 * 2 * n_paths - 2)}
    if not args.no_check:
        for b in sorted({0, B - 1}):  # the first pair, and the last one: the one at the highest address
            i = b % left_np.shape[0]
            want = reference(name, n_paths, i, left_np[i], right_np[i], p.bf, args.disparities)
            assert sg.disparity[b, 0].cpu().numpy().tobytes() == want["disparity"].tobytes(), "the kernels and the restatement disagree"
            assert sg.depth[b, 0].cpu().numpy().tobytes() == want["depth"].tobytes() and int(sg.n_valid[b, 0].item()) == want["n_valid"]
        out["checked"] = True
    if args.once:
        for _ in range(ONCE_CALLS - 1):
            run()
        torch.cuda.synchronize()
        return out
    ds = ops.DenseStereoBatch(B, 1, rows, cols)
    dp = ops.dense_stereo_params(camera, n_disparities=args.disparities)
    half = torch.empty(COPY_BYTES // 2, dtype=torch.uint8, device=dev)
    other = torch.empty_like(half)
    fns = {"call": run, "local": lambda: ds.run(ctx, dp, left, right), "copy": lambda: other.copy_(half)}
    t = interleaved(fns, args.rounds)
    for k, (med, low) in t.items():
        out[k] = {"ms_median": med, "ms_min": low, "us_per_pair": med * 1e3 / B}
    out["local_valid_share"] = float(ds.n_valid.sum().item()) / pixels
    rate = COPY_BYTES / (t["copy"][0] * 1e-3)
    out["floor"] = {"copy_GB_per_s": rate / 1e9, "hbm_ms": out["hbm_bytes"] / rate * 1e3}
    return out


def breakdown(name, B, n_paths, args, in_flight):
    """the per-kernel split of one configuration: this tool again, in a child process under the profiler -> {kernel: microseconds a
    call}, the path kernel's launches told apart by their place in the call's order"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), name,
               "--batch", str(B), "--paths", str(n_paths), "--disparities", str(args.disparities), "--in-flight", str(in_flight), "--once",
               "--no-check", "--no-breakdown"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        split = {}
        for f in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
            rows = [r for r in csv.DictReader(open(f)) if "sgm_" in r["Kernel_Name"] or "dense_census" in r["Kernel_Name"] or
                    "dense_finish" in r["Kernel_Name"]]
            rows.sort(key=lambda r: int(r["Start_Timestamp"]))
            k = 0
            for r in rows:
                n, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                if "sgm_path" in n:
                    short = "path" + DIRECTIONS[k % n_paths]
                    k += 1
                else:
                    short = "winner" if "sgm_winner" in n else "right" if "sgm_right" in n else "census" if "census" in n else "finish"
                split[short] = split.get(short, 0.0) + us / ONCE_CALLS
        return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", default=["kitti", "euroc"])
    ap.add_argument("--batch", nargs="*", type=int, default=[1, 64, 1024])
    ap.add_argument("--paths", nargs="*", type=int, default=[4, 8])
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--in-flight", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--no-breakdown", action="store_true")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sgm_stereo.py measures on the GPU"
    ctx = ops.Context(0)
    results = []
    for name in args.shape:
        for B in args.batch:
            for n_paths in args.paths:
                r = bench(ctx, name, B, n_paths, args)
                results.append(r)
                torch.cuda.empty_cache()
                if "skipped" in r:
                    print("%s x %d, %d paths: skipped (%s)" % (name, B, n_paths, r["skipped"]), flush=True)
                    continue
                line = "%s %d x %d, B = %d, %d disparities, %d paths, %d in flight, %d launches (%.0f %% valid, workspace %.1f MB)" % (
                    name, r["rows"], r["cols"], B, args.disparities, n_paths, r["images_in_flight"], r["launches"], 100 * r["valid_share"],
                    r["workspace_bytes"] / 1e6)
                if "call" in r:
                    line += ": call %.3f ms (min %.3f), %.1f us a pair; local %.3f ms, %.1f us a pair (%.0f %% valid); floor: hbm %.3f ms " \
                            "(%.0f MB at the copy's %.0f GB/s): %.1f x the floor" % (
                                r["call"]["ms_median"], r["call"]["ms_min"], r["call"]["us_per_pair"], r["local"]["ms_median"],
                                r["local"]["us_per_pair"], 100 * r["local_valid_share"], r["floor"]["hbm_ms"], r["hbm_bytes"] / 1e6,
                                r["floor"]["copy_GB_per_s"], r["call"]["ms_median"] / r["floor"]["hbm_ms"])
                print(line, flush=True)
    ctx.close()
    if not args.no_breakdown and not args.once:  # the children open the device after this process has let go of its tensors
        for r in results:
            if "skipped" not in r:
                try:
                    r["kernels_us_per_call"] = breakdown(r["shape"], r["batch"], r["n_paths"], args, r["images_in_flight"])
                except (subprocess.SubprocessError, OSError, KeyError, ValueError) as e:
                    print("%s B = %d, %d paths per kernel: the profiler run failed (%s)" % (r["shape"], r["batch"], r["n_paths"], e), flush=True)
                    continue
                print("%s B = %d, %d paths, us a call per kernel: %s" % (r["shape"], r["batch"], r["n_paths"], ", ".join(
                    "%s %.1f" % (k, v) for k, v in r["kernels_us_per_call"].items())), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
