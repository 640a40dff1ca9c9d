"""Dense RGB-D cloud throughput (prs_depth_cloud_batch_run): B sequences of F 640 x 480 16-bit depth frames resident in HBM, placed in
the world by a seeded trajectory.
usage: python tools/bench_depth_cloud.py [BxF ...] [--step N ...] [--rounds N] [--json FILE] [--no-host] [--once]
  The depth is seeded: four distinct frames of 0.4 .. 6 m in millimetres with a tenth of the pixels 0, replicated over the batch.
  Per shape and step, in one process, timed with events on the stream in interleaved rounds (median and minimum over the rounds):
    cloud      ms per call (count, scan, scatter) and per frame; bytes moved = the depth read once plus the 16-byte rows written (the
               kernels read the depth twice: that is in the time, not in the bytes); xyz alone, no frame or pixel array
    count      the count-only call: its share is the first read of the depth
    copy       a plain device-to-device copy that moves the same number of bytes: the ceiling the call is judged against
    measure    prs_depth_measurements_batch on the same frames with 1000 keypoints each, for scale
    host       the route it replaces: .cpu() of the depth, the numpy restatement (tests/depth_cloud_ref.py) on one frame scaled to
               the frames
  Shapes default to 1x64 64x16 256x4, steps to 1 4.  --once: one call per shape and a comparison with the restatement, no timing
  (for a profiler)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from srrg2_proslam_amd import ops  # noqa: E402

ROWS, COLS = 480, 640
CAMERA = dict(fx=481.2, fy=-481.0, cx=319.5, cy=239.5)  # ICL-NUIM
KEYPOINTS = 1000


def _window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _iters(fn, seconds=0.25):
    """warm up, then the number of calls that fills `seconds`"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return int(min(max(seconds * 1e3 / max(_window(fn, 3), 1e-3), 5), 2000))


def interleaved(fns, rounds):
    """{name: (median ms, min ms)} of every fn, timed round by round in turn"""
    iters = {k: _iters(f) for k, f in fns.items()}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            times[k].append(_window(f, iters[k]))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in times.items()}


def seeded_poses(rng, n):
    """n camera poses along a gentle walk, float32 [n, 16]"""
    out = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        a = 0.02 * i + rng.normal(0, 0.002)
        out[i, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        out[i, :3, 3] = [0.05 * i, rng.normal(0, 0.01), 0.01 * i]
        out[i, 3, 3] = 1
    return out.reshape(n, 16)


def bench(ctx, B, F, step, rounds, host, once):
    import depth_cloud_ref as ref
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    base_np = rng.integers(400, 6000, (4, ROWS, COLS)).astype(np.uint16)
    base_np[rng.random(base_np.shape) < 0.1] = 0
    base = torch.from_numpy(base_np.view(np.int16)).to(dev)  # (no uint16 gather in torch)
    depth = base[torch.arange(B * F, device=dev) % 4].view(torch.uint16).view(B, F, ROWS, COLS)
    pose_np = seeded_poses(rng, F)
    pose = torch.from_numpy(pose_np).to(dev).repeat(B, 1, 1).contiguous()
    n_images = torch.full((B,), F, dtype=torch.int32, device=dev)
    sampled = len(range(0, ROWS, step)) * len(range(0, COLS, step))
    dc = ops.DepthCloudBatch(B, F, ROWS, COLS, F * sampled, outputs=())
    kw = dict(scale=1e-3, step=step)
    p, rp = ops.depth_cloud_params(CAMERA, **kw), ref.params(CAMERA, **kw)
    dc.run(ctx, p, depth, pose, n_images)
    torch.cuda.synchronize()
    rows = int(dc.n_out.sum().item())
    assert int(dc.status.abs().max().item()) == 0 and int(dc.n_total.sum().item()) == rows
    # the first and the last sequence against the restatement
    for b in sorted({0, B - 1}):
        want = ref.depth_cloud(dict(depth=depth[b].cpu().numpy(), n_images=F, pose=pose_np), rp, dc.out_stride)
        assert int(dc.n_out[b].item()) == want["n_out"], "the kernel and the restatement disagree on the count"
        assert dc.xyz[b].cpu().numpy().tobytes() == want["xyz"].tobytes(), "the kernel and the float32 restatement disagree"
    depth_bytes = depth.numel() * 2
    nbytes = depth_bytes + 16 * rows
    out = {"shape": "%dx%d 640x480 u16 step %d" % (B, F, step), "batch": B, "frames": F, "step": step, "rows": rows,
           "kept_share": rows / float(B * F * sampled), "bytes": nbytes, "depth_bytes": depth_bytes}
    if once:
        return out
    fns = {"cloud": lambda: dc.run(ctx, p, depth, pose, n_images), "count": lambda: dc.count(ctx, p, depth, pose, n_images)}
    half = torch.empty((nbytes // 2 + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    other = torch.empty_like(half)
    fns["copy"] = lambda: other.copy_(half)
    flat = depth.view(B * F, ROWS, COLS)
    kp = torch.from_numpy(np.stack([rng.uniform(0, COLS - 1, (KEYPOINTS,)), rng.uniform(0, ROWS - 1, (KEYPOINTS,))], axis=1).astype(np.float32))
    kp = kp.to(dev).repeat(B * F, 1, 1).contiguous()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    desc, fixed, fdesc = z((B * F, KEYPOINTS, 32), torch.uint8), z((B * F, KEYPOINTS, 4), torch.float32), z((B * F, KEYPOINTS, 32), torch.uint8)
    n_feat, n_fixed, st = torch.full((B * F,), KEYPOINTS, dtype=torch.int32, device=dev), z((B * F,), torch.int32), z((B * F,), torch.int32)
    mp = ops.depth_params("u16", 1e-3)
    fns["measure"] = lambda: ops.depth_measurements_batch(ctx, mp, flat, kp, desc, n_feat, fixed, fdesc, n_fixed, st)
    t = interleaved(fns, rounds)
    dc.run(ctx, p, depth, pose, n_images)  # the count-only calls left n_out at 0
    for k, (med, low) in t.items():
        out[k] = {"ms_median": med, "ms_min": low, "us_per_frame": med * 1e3 / (B * F),
                  "GB_per_s": nbytes / (med * 1e-3) / 1e9 if k in ("cloud", "copy") else None}
    if host:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = depth.cpu()
        t1 = time.perf_counter()
        one = h[0, :1].numpy()
        ref.host_route(one, pose_np[:1], rp)
        t2 = time.perf_counter()
        ref.host_route(one, pose_np[:1], rp)
        t3 = time.perf_counter()
        out["host"] = {"download_ms": (t1 - t0) * 1e3, "numpy_ms_per_frame": (t3 - t2) * 1e3, "total_ms": ((t1 - t0) + (t3 - t2) * B * F) * 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", default=["1x64", "64x16", "256x4"])
    ap.add_argument("--step", nargs="*", type=int, default=[1, 4])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_cloud.py measures on the GPU"
    ctx = ops.Context(0)
    results = []
    for shape in args.shape:
        B, F = (int(x) for x in shape.lower().split("x"))
        for step in args.step:
            r = bench(ctx, B, F, step, args.rounds, not args.no_host, args.once)
            results.append(r)
            line = "%s (%d rows, %.1f %% kept, %.1f MB depth + rows):" % (r["shape"], r["rows"], 100 * r["kept_share"], r["bytes"] / 1e6)
            for k, v in r.items():
                if isinstance(v, dict) and "ms_median" in v:
                    line += "  %s %.4f ms (min %.4f, %.2f us a frame)" % (k, v["ms_median"], v["ms_min"], v["us_per_frame"])
                    line += ", %.0f GB/s" % v["GB_per_s"] if v["GB_per_s"] else ""
            print(line, flush=True)
            if "copy" in r:
                print("    the call takes %.2f x the copy of its bytes, %.2f x the measurement stage; count-only is %.0f %% of it" % (
                    r["cloud"]["ms_median"] / r["copy"]["ms_median"], r["cloud"]["ms_median"] / r["measure"]["ms_median"],
                    100 * r["count"]["ms_median"] / r["cloud"]["ms_median"]), flush=True)
            if "host" in r:
                h = r["host"]
                print("    host route: download %.1f ms + numpy %.1f ms a frame x %d = %.0f ms" % (
                    h["download_ms"], h["numpy_ms_per_frame"], B * F, h["total_ms"]), flush=True)
            torch.cuda.empty_cache()
    ctx.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
