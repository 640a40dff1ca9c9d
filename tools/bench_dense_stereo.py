"""Dense stereo throughput (prs_dense_stereo_batch_run): B rectified pairs resident in HBM to disparity and depth images.
usage: python tools/bench_dense_stereo.py [kitti|euroc ...] [--batch N ...] [--disparities N] [--radius N] [--rounds N] [--json FILE]
                                          [--no-breakdown] [--no-check] [--once]
  Shapes: kitti 376 x 1241, euroc 480 x 752; batches default to 1 64 1024 (a batch that does not fit the free memory is skipped).
  The pairs are seeded: four distinct right images of random bytes, the left ones shifted by a disparity that changes from band to
  band of rows, replicated over the batch.  The first and the last pair are compared with the restatement (tests/dense_stereo_ref.py) byte for byte.
  Per shape and batch, timed with events on the stream in interleaved rounds (median and minimum over the rounds):
    call       ms per call (census, left match, right match, finish) and us per pair
    no lr      the call with lr_max_diff = -1: without the right match and its winners
    copy       a device-to-device copy of the call's HBM bytes, for the first floor
  and against them the two floors:
    hbm        the bytes a call cannot avoid -- per pixel 2 in, 8 out, the census words written (16) and read by each match pass
               (2 x 16), the left records written and read (16), the right winners written and read (4): 78 -- at the bandwidth the
               copy reached
    issue      the popcount, xor and add instructions the match kernels issue: per staged column, pair of disparities and row
               8 v_xor + 8 v_bcnt (two 64-bit popcounts entering, two leaving), 4 to pack and apply them, 2 r + 1 adds for the box
               sum and 6 for the two packed minima, over both passes, at 2 cycles a wave instruction on every SIMD at the device's
               clock.  LDS traffic is not in it
  --breakdown (default): the configuration once more in a child process of its own under `rocprofv3 --kernel-trace --stats`, for
  the time per kernel.  --once: five calls and no timing (what the child runs)."""
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

SHAPES = {"kitti": (376, 1241, configs.KITTI["camera"]), "euroc": (480, 752, configs.EUROC["camera"])}
HBM_BYTES_PER_PIXEL = 2 + 8 + 16 + 32 + 16 + 4
BAND, WAVE = 32, 64  # the match kernel's band of rows and its staged columns


def _window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _iters(fn, seconds=0.25):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    return int(min(max(seconds * 1e3 / max(_window(fn, 2), 1e-3), 3), 1000))


def interleaved(fns, rounds):
    """{name: (median ms, min ms)} of every fn, timed round by round in turn"""
    iters = {k: _iters(f) for k, f in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            times[k].append(_window(f, iters[k]))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in times.items()}


def seeded_pairs(rows, cols, n=4):
    rng = np.random.default_rng(3)
    right = rng.integers(0, 256, (n, rows, cols), dtype=np.uint8)
    left = np.empty_like(right)
    xs = np.arange(cols)
    for v0 in range(0, rows, 47):
        d = 5 + (v0 * 7) % 96
        left[:, v0:v0 + 47] = right[:, v0:v0 + 47][:, :, np.clip(xs - d, 0, cols - 1)]
    return left, right


def issue_floor_instructions(rows, cols, n_disparities, r):
    """wave instructions of the arithmetic listed above, both match passes of one pair"""
    tile = WAVE - 2 * r
    tiles, bands = -(-cols // tile), -(-rows // BAND)
    row_steps = rows + bands * 2 * r  # a band's first row adds 2 r + 1 rows
    pairs = (n_disparities + 1) // 2
    return 2 * tiles * pairs * (row_steps * 20 + rows * (2 * r + 1 + 6))


def bench(ctx, name, B, args):
    import dense_stereo_ref as ref
    rows, cols, camera = SHAPES[name]
    dev = torch.device("cuda", 0)
    pixels = B * rows * cols
    need = pixels * (2 + 8 + 26) + 2 * pixels * HBM_BYTES_PER_PIXEL // 2
    free = torch.cuda.mem_get_info()[0]
    if need > 0.8 * free or pixels > 2 ** 31 - 1:
        return {"shape": name, "batch": B, "skipped": "needs %.1f GB, %.1f GB free" % (need / 1e9, free / 1e9)}
    left_np, right_np = seeded_pairs(rows, cols)
    pick = torch.arange(B, device=dev) % left_np.shape[0]
    left = torch.from_numpy(left_np).to(dev)[pick].view(B, 1, rows, cols)
    right = torch.from_numpy(right_np).to(dev)[pick].view(B, 1, rows, cols)
    ds = ops.DenseStereoBatch(B, 1, rows, cols)
    kw = dict(n_disparities=args.disparities, aggregation_radius=args.radius)
    p, p_nolr = ops.dense_stereo_params(camera, **kw), ops.dense_stereo_params(camera, lr_max_diff=-1, **kw)
    run = lambda: ds.run(ctx, p, left, right)  # noqa: E731
    run()
    torch.cuda.synchronize()
    assert int(ds.status.abs().max().item()) == 0
    out = {"shape": name, "rows": rows, "cols": cols, "batch": B, "n_disparities": args.disparities, "aggregation_radius": args.radius,
           "valid_share": float(ds.n_valid.sum().item()) / pixels, "workspace_bytes": int(ds.workspace.numel()),
           "hbm_bytes": pixels * HBM_BYTES_PER_PIXEL}
    if not args.no_check:
        for b in sorted({0, B - 1}):  # the first pair, and the last one: the one at the highest address
            i = b % left_np.shape[0]
            want = ref.dense_stereo_image(left_np[i], right_np[i], ref.params(p.bf, args.disparities, 0, args.radius, 10, 1))
            assert ds.disparity[b, 0].cpu().numpy().tobytes() == want["disparity"].tobytes(), "the kernels and the restatement disagree"
            assert ds.depth[b, 0].cpu().numpy().tobytes() == want["depth"].tobytes() and int(ds.n_valid[b, 0].item()) == want["n_valid"]
        out["checked"] = True
    if args.once:
        for _ in range(4):
            run()
        torch.cuda.synchronize()
        return out
    half = torch.empty((out["hbm_bytes"] // 2 + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    other = torch.empty_like(half)
    fns = {"call": run, "no_lr": lambda: ds.run(ctx, p_nolr, left, right), "copy": lambda: other.copy_(half)}
    t = interleaved(fns, args.rounds)
    for k, (med, low) in t.items():
        out[k] = {"ms_median": med, "ms_min": low, "us_per_pair": med * 1e3 / B}
    props = torch.cuda.get_device_properties(0)
    clock_hz = getattr(props, "clock_rate", 2400000) * 1e3  # kHz; 2.4 GHz, the MI355X's peak engine clock, where torch does not report one
    instr = B * issue_floor_instructions(rows, cols, args.disparities, args.radius)
    out["floors"] = {"hbm_ms": t["copy"][0], "copy_GB_per_s": out["hbm_bytes"] / (t["copy"][0] * 1e-3) / 1e9, "issue_wave_instructions": instr,
                     "issue_ms": instr * 2 / (props.multi_processor_count * 4 * clock_hz) * 1e3, "compute_units": props.multi_processor_count,
                     "clock_GHz": clock_hz / 1e9}
    return out


def breakdown(name, B, args):
    """the per-kernel split of one configuration: this tool again, in a child process under the profiler -> {kernel: microseconds}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), name,
               "--batch", str(B), "--disparities", str(args.disparities), "--radius", str(args.radius), "--once", "--no-check", "--no-breakdown"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        split = {}
        for f in glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                n = r["Name"]
                if "dense_" in n and "_kernel" in n:
                    short = n[n.index("dense_"):].split("(")[0]
                    short = short[:short.index("_kernel")] + ("<right>" if "ILb1E" in n or "<true" in n else "<left>" if "match" in short else "")
                    split[short] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3}
        return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", default=["kitti", "euroc"])
    ap.add_argument("--batch", nargs="*", type=int, default=[1, 64, 1024])
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--no-breakdown", action="store_true")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dense_stereo.py measures on the GPU"
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
            line = "%s %d x %d, B = %d, %d disparities, r = %d (%.0f %% valid, workspace %.1f MB)" % (
                name, r["rows"], r["cols"], B, args.disparities, args.radius, 100 * r["valid_share"], r["workspace_bytes"] / 1e6)
            if "call" in r:
                fl = r["floors"]
                line += ": call %.3f ms (min %.3f), %.1f us a pair; no lr %.3f ms; floors: hbm %.3f ms (%.0f MB at the copy's %.0f GB/s), " \
                        "issue %.3f ms (%.3g wave instructions, %d CUs at %.2f GHz)" % (
                            r["call"]["ms_median"], r["call"]["ms_min"], r["call"]["us_per_pair"], r["no_lr"]["ms_median"], fl["hbm_ms"],
                            r["hbm_bytes"] / 1e6, fl["copy_GB_per_s"], fl["issue_ms"], fl["issue_wave_instructions"], fl["compute_units"],
                            fl["clock_GHz"])
            print(line, flush=True)
    ctx.close()
    if not args.no_breakdown and not args.once:  # the children open the device after this process has let go of its tensors
        for r in results:
            if "skipped" not in r:
                try:
                    r["kernels"] = breakdown(r["shape"], r["batch"], args)
                except (subprocess.SubprocessError, OSError) as e:
                    print("%s B = %d per kernel: the profiler run failed (%s)" % (r["shape"], r["batch"], e), flush=True)
                    continue
                print("%s B = %d per kernel: %s" % (r["shape"], r["batch"], ", ".join(
                    "%s %.1f us" % (k, v["average_us"]) for k, v in sorted(r["kernels"].items()))), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
