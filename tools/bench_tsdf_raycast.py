"""TSDF raycast throughput (prs_tsdf_raycast_batch_run): B sequences of V views of 640 x 480 pixels rendered out of one N x N x N
volume a sequence, everything resident in HBM.
usage: python tools/bench_tsdf_raycast.py [BxVxN ...] [--rounds N] [--json FILE] [--once]
  The volumes are those of tools/bench_tsdf.py: V seeded 16-bit depth frames of a rolling surface between 1.5 and 3.5 m, seen along a
  gentle walk, fused into a cube of 4 m in front of the first camera (voxel = 4 m / N, truncation = 4 voxels).  The views are rendered
  from the poses the frames were taken at, with a step of one voxel.  Per shape, in one process, timed with events on the stream in
  interleaved rounds (median and minimum over the rounds), per call and per view:
    raycast    depth, normal and n_hit of every view
    copy       (a) a device-to-device copy that moves the output's bytes (20 a pixel): the traffic the call cannot avoid
    surface    (b) prs_tsdf_surface_batch_run on the same volumes: the other reader of the volume
    integrate  (c) prs_tsdf_integrate_batch_run of as many images into the same volumes: the stage the raycast inverts
  Shapes default to 1x64x256 64x16x128 256x4x64.  Rows 0, 239 and 479 of the first view of the first and of the last sequence are
  compared with the numpy restatement byte for byte.  --once: one call and those comparisons, no timing (for a profiler)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from srrg2_proslam_amd import configs, ops  # noqa: E402
from bench_depth_cloud import interleaved, seeded_poses  # noqa: E402
from bench_depth_normals import seeded_depth  # noqa: E402

ROWS, COLS, SCALE = 480, 640, 1e-3
CAMERA = dict(fx=481.2, fy=-481.0, cx=319.5, cy=239.5)  # ICL-NUIM
EXTENT = 4.0
CHECKED_ROWS = (0, 239, 479)


def bench(ctx, B, V, N, rounds, once):
    import tsdf_raycast_ref as ref
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    base = torch.from_numpy(seeded_depth(rng, ROWS, COLS, "u16").view(np.int16)).to(dev)  # (no uint16 gather in torch)
    frames = base[torch.arange(B * V, device=dev) % 4].view(torch.uint16).view(B, V, ROWS, COLS)
    pose_np = seeded_poses(rng, V)
    pose = torch.from_numpy(pose_np).to(dev).repeat(B, 1, 1).contiguous()
    vs = EXTENT / N
    fp = ops.tsdf_params(CAMERA, voxel_size=vs, truncation=4 * vs, scale=SCALE)
    voxels = N * N * N
    cap = min(voxels // 2, 8 << 20)
    vb = ops.TsdfVolumeBatch(B, N, N, N, V, ROWS, COLS, out_stride=cap)
    origin_np = np.array([-EXTENT / 2, -EXTENT / 2, 0.5, 0.0], np.float32)
    vb.origin.copy_(torch.from_numpy(np.tile(origin_np, (B, 1))))
    vb.integrate(ctx, fp, frames, pose)
    kw = dict(voxel_size=vs, step=vs, min_weight=configs.TSDF_RAYCAST["min_weight"], range_min=configs.TSDF_RAYCAST["range_min"],
              range_max=configs.TSDF_RAYCAST["range_max"])
    p, rp = ops.tsdf_raycast_params(CAMERA, **kw), ref.params(CAMERA, **kw)
    rb = ops.TsdfRaycastBatch(ctx, vb, V, ROWS, COLS)
    depth, normal, n_hit = rb.run(p, pose)
    torch.cuda.synchronize()
    assert int(rb.status.abs().max().item()) == 0 and int(rb.n_skipped.abs().max().item()) == 0
    hits, with_normal = int(n_hit.sum().item()), int((normal[..., 3] > 0).sum().item())
    v, u = np.meshgrid(np.array(CHECKED_ROWS), np.arange(COLS), indexing="ij")
    rows = torch.tensor(CHECKED_ROWS, device=dev)
    for b in sorted({0, B - 1}):
        want = ref.raycast(dict(pose=pose_np[:1]), rp, origin_np, vb.volume[b].cpu().numpy(), 1, ROWS, COLS, pixels=(v, u))
        assert depth[b, 0, rows].cpu().numpy().tobytes() == want["depth"][0].tobytes() and \
            normal[b, 0, rows].cpu().numpy().tobytes() == want["normal"][0].tobytes(), "the kernel and the float32 restatement disagree"
    pixels = B * V * ROWS * COLS
    out = {"shape": "%dx%d vga views out of %d^3" % (B, V, N), "batch": B, "views": V, "n": N, "pixels": pixels, "hits": hits,
           "hit_share": hits / float(pixels), "normal_share": with_normal / float(max(hits, 1)), "output_bytes": pixels * 20,
           "volume_bytes": B * voxels * 8}
    if once:
        return out
    half = torch.empty(((pixels * 10 + 15) // 16 * 16,), dtype=torch.uint8, device=dev)
    other = torch.empty_like(half)
    saved = vb.volume.clone()
    fns = {"raycast": lambda: rb.run(p, pose), "copy": lambda: other.copy_(half), "surface": lambda: vb.surface(ctx, fp),
           "integrate": lambda: vb.integrate(ctx, fp, frames, pose)}
    t = interleaved(fns, rounds)
    vb.volume.copy_(saved)
    for k, (med, low) in t.items():
        out[k] = {"ms_median": med, "ms_min": low, "us_per_view": med * 1e3 / (B * V)}
    out["raycast"]["Mrays_per_s"] = pixels / (t["raycast"][0] * 1e-3) / 1e6
    out["copy"]["GB_per_s"] = out["output_bytes"] / (t["copy"][0] * 1e-3) / 1e9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", default=["1x64x256", "64x16x128", "256x4x64"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tsdf_raycast.py measures on the GPU"
    ctx = ops.Context(0)
    results = []
    for shape in args.shape:
        B, V, N = (int(x) for x in shape.lower().split("x"))
        r = bench(ctx, B, V, N, args.rounds, args.once)
        results.append(r)
        line = "%s (%.1f %% of the pixels hit, %.1f %% of those with a normal, output %.1f MB, volumes %.1f MB):" % (
            r["shape"], 100 * r["hit_share"], 100 * r["normal_share"], r["output_bytes"] / 1e6, r["volume_bytes"] / 1e6)
        for k in ("raycast", "copy", "surface", "integrate"):
            if k in r:
                line += "  %s %.4f ms (min %.4f, %.2f us a view)" % (k, r[k]["ms_median"], r[k]["ms_min"], r[k]["us_per_view"])
        print(line, flush=True)
        if "copy" in r:
            print("    %.0f Mrays/s; raycast takes %.2f x the copy of its output, %.2f x the surface call and %.2f x the integrate call" % (
                r["raycast"]["Mrays_per_s"], r["raycast"]["ms_median"] / r["copy"]["ms_median"],
                r["raycast"]["ms_median"] / r["surface"]["ms_median"], r["raycast"]["ms_median"] / r["integrate"]["ms_median"]), flush=True)
        torch.cuda.empty_cache()
    ctx.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
