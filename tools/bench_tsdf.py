"""TSDF fusion throughput (prs_tsdf_integrate_batch_run, prs_tsdf_surface_batch_run): B sequences of F depth frames resident in HBM,
640 x 480 16-bit millimetres, fused into one N x N x N volume a sequence.
usage: python tools/bench_tsdf.py [BxFxN ...] [--rounds N] [--json FILE] [--no-torch] [--once]
  The depth is seeded: four distinct frames of a rolling surface between 1.5 and 3.5 m with a 40 cm step every 97 columns and 61 rows
  and a tenth of the pixels 0, replicated over the batch, seen along a gentle walk; the volume is a cube of 4 m in front of the first
  camera (voxel = 4 m / N, truncation = 4 voxels).  Per shape, in one process, timed with events on the stream in interleaved rounds
  (median and minimum over the rounds):
    integrate  ms per call into a volume that holds an earlier call's result (the steady state) and per image
    copy       (a) a device-to-device copy of the volume's bytes: 8 read and 8 written a voxel, the call's traffic floor
    cloud      (b) prs_depth_cloud_batch_run (xyz alone) followed by prs_world_voxel_batch_run at the same voxel size on the same
               frames: the route the fusion stands beside
    torch      (c) the rule written with torch ops on the device, a sequence and an image at a time: what a user has today.  Timed
               once warm; its volume is compared with the kernel's (bytes, and the largest difference)
    surface    ms per call with xyz, normal and cell; surface copy: a device-to-device copy of the volume's bytes read once (8 a voxel)
               plus the rows written
  Shapes default to 1x64x256 64x16x128 256x4x64.  The first and the last sequence are compared with the numpy restatement byte for
  byte on a slab of four layers through the volume's middle, and the surface's rows of a volume of 64^3 in whole.  --once: one call
  per entry point and those comparisons, no timing (for a profiler)."""
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


def torch_rule(volume, origin, depth, Ti, p):
    """the rule of include/proslam_hip_tsdf.h with torch ops: volume [nz, ny, nx, 2] in place, one image after the other"""
    nz, ny, nx = volume.shape[:3]
    dev, f32 = volume.device, torch.float32
    vs = p.voxel_size
    c0 = (origin[0] + (torch.arange(nx, device=dev, dtype=f32) + 0.5) * vs)[None, None, :]
    c1 = (origin[1] + (torch.arange(ny, device=dev, dtype=f32) + 0.5) * vs)[None, :, None]
    c2 = (origin[2] + (torch.arange(nz, device=dev, dtype=f32) + 0.5) * vs)[:, None, None]
    tsdf, w = volume[..., 0], volume[..., 1]
    for f in range(depth.shape[0]):
        T = Ti[f]
        q = [((T[i, 0] * c0 + T[i, 1] * c1) + T[i, 2] * c2) + T[i, 3] for i in range(3)]
        z = q[2].expand(nz, ny, nx)
        m = (z > 0) & (z >= p.range_min) & (z <= p.range_max)
        uf = torch.floor((q[0] / z * p.fx + p.cx) + 0.5)
        vf = torch.floor((q[1] / z * p.fy + p.cy) + 0.5)
        m = m & (uf >= 0) & (uf < COLS) & (vf >= 0) & (vf < ROWS)
        u, v = torch.where(m, uf, torch.zeros_like(uf)).long(), torch.where(m, vf, torch.zeros_like(vf)).long()
        raw = depth[f][v, u].to(f32)
        d = p.depth_scaling_factor_to_meters * raw
        m = m & (raw > 0) & (d >= p.range_min) & (d <= p.range_max)
        sdf = d - z
        m = m & (sdf >= -p.truncation)
        t = torch.clamp(sdf / p.truncation, max=1.0)
        w1 = w + 1.0
        tsdf.copy_(torch.where(m, (tsdf * w + t) / w1, tsdf))
        w.copy_(torch.where(m, torch.clamp(w1, max=p.max_weight), w))
    return volume


def bench(ctx, B, F, N, rounds, with_torch, once):
    import tsdf_ref as ref
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    base_np = seeded_depth(rng, ROWS, COLS, "u16")
    base = torch.from_numpy(base_np.view(np.int16)).to(dev)  # (no uint16 gather in torch)
    depth = base[torch.arange(B * F, device=dev) % 4].view(torch.uint16).view(B, F, ROWS, COLS)
    pose_np = seeded_poses(rng, F)
    pose = torch.from_numpy(pose_np).to(dev).repeat(B, 1, 1).contiguous()
    n_images = torch.full((B,), F, dtype=torch.int32, device=dev)
    vs = EXTENT / N
    kw = dict(voxel_size=vs, truncation=4 * vs, max_weight=configs.TSDF["max_weight"], min_weight=configs.TSDF["min_weight"],
              range_min=configs.TSDF["range_min"], range_max=configs.TSDF["range_max"], scale=SCALE)
    p, rp = ops.tsdf_params(CAMERA, **kw), ref.params(CAMERA, **kw)
    voxels = N * N * N
    cap = min(voxels // 2, 8 << 20)
    vb = ops.TsdfVolumeBatch(B, N, N, N, F, ROWS, COLS, out_stride=cap)
    origin_np = np.array([-EXTENT / 2, -EXTENT / 2, 0.5, 0.0], np.float32)
    vb.origin.copy_(torch.from_numpy(np.tile(origin_np, (B, 1))))
    vb.integrate(ctx, p, depth, pose, n_images)
    xyz, normal, n_out = vb.surface(ctx, p)
    torch.cuda.synchronize()
    assert int(vb.status.abs().max().item()) == 0 and int(vb.n_skipped.abs().max().item()) == 0
    updates = int(vb.n_updates.sum().item())
    crossings = int(vb.n_total.sum().item())
    host_depth, k0 = depth[0].cpu().numpy(), N // 2 - 2
    for b in sorted({0, B - 1}):  # the sequences hold the same images
        want = ref.integrate(dict(depth=host_depth, pose=pose_np), rp, origin_np, np.zeros((4, N, N, 2), np.float32), slab=(k0, k0 + 4))
        assert vb.volume[b, k0:k0 + 4].cpu().numpy().tobytes() == want["volume"].tobytes(), "the kernel and the float32 restatement disagree"
        if N <= 64:
            rows = ref.surface(vb.volume[b].cpu().numpy(), rp, origin_np, cap)
            n = rows["n_out"]
            assert int(n_out[b].item()) == n and xyz[b, :n].cpu().numpy().tobytes() == rows["xyz"][:n].tobytes() and \
                normal[b, :n].cpu().numpy().tobytes() == rows["normal"][:n].tobytes(), "the surface and the restatement disagree"
    out = {"shape": "%dx%d vga u16 into %d^3" % (B, F, N), "batch": B, "frames": F, "n": N, "voxels": B * voxels, "updates": updates,
           "update_share": updates / float(B * F * voxels), "crossings": crossings, "capacity_hit": bool((vb.surface_status != 0).any().item()),
           "volume_bytes": B * voxels * 8}
    if once:
        return out
    half, other = torch.empty_like(vb.volume), torch.empty_like(vb.volume)
    surf_bytes = B * voxels * 8 + int(n_out.sum().item()) * 36
    s_half = torch.empty(((surf_bytes // 2 + 15) // 16 * 16,), dtype=torch.uint8, device=dev)
    s_other = torch.empty_like(s_half)
    dc = ops.DepthCloudBatch(B, F, ROWS, COLS, F * ROWS * COLS, outputs=())
    cp = ops.depth_cloud_params(CAMERA, range_min=kw["range_min"], range_max=kw["range_max"], scale=SCALE)
    dc.run(ctx, cp, depth, pose, n_images)
    wv = ops.WorldVoxelBatch(B, F * ROWS * COLS, F * ROWS * COLS, outputs=())
    vp = ops.world_voxel_params(vs)

    def route():
        dc.run(ctx, cp, depth, pose, n_images)
        wv.run(ctx, vp, dc)

    fns = {"integrate": lambda: vb.integrate(ctx, p, depth, pose, n_images), "copy": lambda: other.copy_(half), "cloud": route,
           "surface": lambda: vb.surface(ctx, p), "surface_copy": lambda: s_other.copy_(s_half)}
    saved = vb.volume.clone()
    t = interleaved(fns, rounds)
    vb.volume.copy_(saved)
    for k, (med, low) in t.items():
        out[k] = {"ms_median": med, "ms_min": low, "us_per_image": med * 1e3 / (B * F)}
    out["integrate"]["GB_per_s"] = 2 * out["volume_bytes"] / (t["integrate"][0] * 1e-3) / 1e9
    out["copy"]["GB_per_s"] = 2 * out["volume_bytes"] / (t["copy"][0] * 1e-3) / 1e9
    del half, other, s_half, s_other, dc, wv
    if with_torch:
        S = np.eye(4, dtype=np.float32)
        Ti = torch.from_numpy(np.stack([ref.se3_inverse(ref.se3_mul(P.reshape(4, 4), S)) for P in pose_np])).to(dev)
        scratch = torch.zeros((N, N, N, 2), dtype=torch.float32, device=dev)
        d16 = depth[0].view(torch.int16).to(torch.int32) & 0xffff
        origin = [float(x) for x in origin_np[:3]]
        torch_rule(scratch, origin, d16, Ti, p)
        scratch.zero_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_rule(scratch, origin, d16, Ti, p)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) * B  # a sequence at a time
        vb.clear()
        vb.integrate(ctx, p, depth, pose, n_images)
        torch.cuda.synchronize()
        out["torch"] = {"ms": ms, "same_bytes": bool(torch.equal(vb.volume[0], scratch)),
                        "max_abs_diff": float((vb.volume[0] - scratch).abs().max().item())}
        del scratch
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", default=["1x64x256", "64x16x128", "256x4x64"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tsdf.py measures on the GPU"
    ctx = ops.Context(0)
    results = []
    for shape in args.shape:
        B, F, N = (int(x) for x in shape.lower().split("x"))
        r = bench(ctx, B, F, N, args.rounds, not args.no_torch, args.once)
        results.append(r)
        line = "%s (%.1f %% of voxel-images update, %d crossings%s, volume %.1f MB):" % (
            r["shape"], 100 * r["update_share"], r["crossings"], ", CAPACITY" if r["capacity_hit"] else "", r["volume_bytes"] / 1e6)
        for k in ("integrate", "copy", "cloud", "surface", "surface_copy"):
            if k in r:
                line += "  %s %.4f ms (min %.4f, %.2f us an image)" % (k, r[k]["ms_median"], r[k]["ms_min"], r[k]["us_per_image"])
                line += ", %.0f GB/s" % r[k]["GB_per_s"] if r[k].get("GB_per_s") else ""
        print(line, flush=True)
        if "copy" in r:
            print("    integrate takes %.2f x the copy of the volume and %.2f x the cloud + voxel-filter route; surface takes %.2f x its copy" % (
                r["integrate"]["ms_median"] / r["copy"]["ms_median"], r["integrate"]["ms_median"] / r["cloud"]["ms_median"],
                r["surface"]["ms_median"] / r["surface_copy"]["ms_median"]), flush=True)
        if "torch" in r:
            t = r["torch"]
            print("    torch ops: %.2f ms, %.0f x the call; same bytes %s, largest difference %g" % (
                t["ms"], t["ms"] / r["integrate"]["ms_median"], t["same_bytes"], t["max_abs_diff"]), flush=True)
        torch.cuda.empty_cache()
    ctx.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
