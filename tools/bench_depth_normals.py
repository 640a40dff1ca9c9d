"""Depth normals throughput (prs_depth_normals_batch_run): B sequences of F depth frames resident in HBM, 640 x 480 16-bit millimetres
(vga) and 1241 x 376 float32 metres (kitti, what the stereo matchers write).
usage: python tools/bench_depth_normals.py [BxF ...] [--image vga kitti] [--radius N ...] [--smooth N ...] [--rounds N] [--json FILE]
                                           [--no-torch] [--once]
  The depth is seeded: four distinct frames of a rolling surface between 1.5 and 3.5 m with a 40 cm step every 97 columns and 61 rows
  and a tenth of the pixels 0, replicated over the batch.  Per shape, image kind and (radius, smooth), in one process, timed with
  events on the stream in interleaved rounds (median and minimum over the rounds):
    normals    ms per call without cloud rows (head and tiles) and per image; bytes moved = the depth read once (2 or 4 bytes a pixel)
               plus the 16-byte normals written
    rows       the same call with one world-frame normal per row of the dense cloud of the same images; `rows kernel` is the
               difference of the two, the third launch
    copy       (a) a plain device-to-device copy that moves the same number of bytes as `normals`: the floor
    cloud      (b) prs_depth_cloud_batch_run on the same images, step 1, xyz with frame and pixel
    torch      (c) the same rule written with torch ops on the device, 16 images at a time: what a user has today.  Timed at
               (1, 0), (2, 1) and (8, 3) only, once warm; its normals are compared with the kernel's (the angle, not the bytes)
  Shapes default to 1x64 64x16 256x4, radius to 1 2 8, smooth to 0 1 3.  The first image of the first and of the last sequence is
  compared with the numpy restatement byte for byte at every setting.  --once: one call per setting and that comparison, no timing
  (for a profiler)."""
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

IMAGES = {
    "vga": dict(rows=480, cols=640, depth_type="u16", scale=1e-3, camera=dict(fx=481.2, fy=-481.0, cx=319.5, cy=239.5)),  # ICL-NUIM
    "kitti": dict(rows=376, cols=1241, depth_type="f32", scale=1.0, camera={k: configs.KITTI["camera"][k] for k in ("fx", "fy", "cx", "cy")}),
}
TORCH_SETTINGS = ((1, 0), (2, 1), (8, 3))
TORCH_CHUNK = 16


def seeded_depth(rng, rows, cols, depth_type):
    """four frames [4, rows, cols] of the depth type"""
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    frames = []
    for i in range(4):
        d = 2.5 + 0.6 * np.sin(u / 40.0 + i) + 0.4 * np.cos(v / 30.0 - i) + 0.4 * ((u // 97 + v // 61) % 2) + rng.normal(0, 0.002, (rows, cols))
        d[rng.random((rows, cols)) < 0.1] = 0.0
        frames.append(d)
    d = np.stack(frames)
    return np.rint(d * 1000.0).astype(np.uint16) if depth_type == "u16" else d.astype(np.float32)


def shifted(a, dv, du, fill):
    """a[..., v + dv, u + du] with `fill` outside, on the device"""
    rows, cols = a.shape[-2:]
    out = torch.full_like(a, fill)
    v0, v1, u0, u1 = max(0, -dv), min(rows, rows - dv), max(0, -du), min(cols, cols - du)
    if v0 < v1 and u0 < u1:
        out[..., v0:v1, u0:u1] = a[..., v0 + dv:v1 + dv, u0 + du:u1 + du]
    return out


def torch_rule(depth, im, radius, smooth, max_rel_diff, range_min, range_max, out):
    """the rule of include/proslam_hip_normals.h with torch ops, TORCH_CHUNK images at a time; depth [N, rows, cols] -> out
    [N, rows, cols, 4]"""
    cam, nan = im["camera"], float("nan")
    rows, cols = depth.shape[-2:]
    kx = ((torch.arange(cols, device=depth.device, dtype=torch.float32) - cam["cx"]) / cam["fx"])[None, None, :]
    ky = ((torch.arange(rows, device=depth.device, dtype=torch.float32) - cam["cy"]) / cam["fy"])[None, :, None]
    for at in range(0, depth.shape[0], TORCH_CHUNK):
        raw = depth[at:at + TORCH_CHUNK].to(torch.float32)
        d = im["scale"] * raw
        d = torch.where((raw > 0) & (d >= range_min) & (d <= range_max), d, torch.full_like(d, nan))
        gate = max_rel_diff * d
        P = torch.stack([kx * d, ky * d, d])

        def neighbour(dv, du):
            return (shifted(d, dv, du, nan) - d).abs() <= gate, shifted(P, dv, du, nan)

        (ul, PL), (ur, PR), (uu, PU), (ud, PD) = neighbour(0, -radius), neighbour(0, radius), neighbour(-radius, 0), neighbour(radius, 0)
        tx = torch.where(ur, PR, P) - torch.where(ul, PL, P)
        ty = torch.where(ud, PD, P) - torch.where(uu, PU, P)
        m = torch.stack([ty[1] * tx[2] - ty[2] * tx[1], ty[2] * tx[0] - ty[0] * tx[2], ty[0] * tx[1] - ty[1] * tx[0]])
        len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
        has = (ul | ur) & (uu | ud) & (len2 > 0) & (len2 <= torch.finfo(torch.float32).max)
        n = m / len2.sqrt()
        dot = (n[0] * P[0] + n[1] * P[1]) + n[2] * P[2]
        n = torch.where(has, torch.where(dot > 0, -n, n), torch.zeros_like(n))
        w = torch.where(has, (ul.to(torch.float32) + ur + uu + ud), torch.zeros_like(d))
        if smooth > 0:
            acc = torch.zeros_like(n)
            for dv in range(-smooth, smooth + 1):
                for du in range(-smooth, smooth + 1):
                    use = shifted(has, dv, du, False) & ((shifted(d, dv, du, nan) - d).abs() <= gate)
                    acc = torch.where(use, acc + shifted(n, dv, du, 0.0), acc)
            len2 = (acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]
            has = has & (len2 > 0) & (len2 <= torch.finfo(torch.float32).max)
            n = torch.where(has, acc / len2.sqrt(), torch.zeros_like(acc))
            w = torch.where(has, w, torch.zeros_like(w))
        out[at:at + TORCH_CHUNK] = torch.cat([n, w[None]]).permute(1, 2, 3, 0)
    return out


def bench(ctx, B, F, kind, settings, rounds, with_torch, once):
    import depth_normals_ref as ref
    im = IMAGES[kind]
    rows, cols, u16 = im["rows"], im["cols"], im["depth_type"] == "u16"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    base_np = seeded_depth(rng, rows, cols, im["depth_type"])
    base = torch.from_numpy(base_np.view(np.int16) if u16 else base_np).to(dev)  # (no uint16 gather in torch)
    depth = base[torch.arange(B * F, device=dev) % 4]
    depth = (depth.view(torch.uint16) if u16 else depth).view(B, F, rows, cols)
    pose_np = seeded_poses(rng, F)
    pose = torch.from_numpy(pose_np).to(dev).repeat(B, 1, 1).contiguous()
    n_images = torch.full((B,), F, dtype=torch.int32, device=dev)
    pixels = B * F * rows * cols
    stride = F * rows * cols
    nb = ops.DepthNormalsBatch(B, F, rows, cols, row_stride=stride)
    dc = ops.DepthCloudBatch(B, F, rows, cols, stride)
    ckw = dict(range_min=configs.DEPTH_NORMALS["range_min"], range_max=configs.DEPTH_NORMALS["range_max"], scale=im["scale"])
    cp = ops.depth_cloud_params(im["camera"], depth_type=im["depth_type"], **ckw)
    dc.run(ctx, cp, depth, pose, n_images)
    torch.cuda.synchronize()
    cloud_rows = int(dc.n_out.sum().item())
    nbytes = depth.numel() * depth.element_size() + 16 * pixels
    half = torch.empty((nbytes // 2 + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    other = torch.empty_like(half)
    results = []
    for radius, smooth in settings:
        nkw = dict(radius=radius, smooth=smooth, max_rel_diff=configs.DEPTH_NORMALS["max_rel_diff"])
        p = ops.depth_normals_params(im["camera"], depth_type=im["depth_type"], **nkw, **ckw)
        rp = ref.params(im["camera"], **nkw, **ckw)
        nb.run(ctx, p, depth, pose, n_images, cloud=dc)
        torch.cuda.synchronize()
        assert int(nb.status.abs().max().item()) == 0 and int(nb.n_bad_rows.abs().max().item()) == 0
        found = int(nb.n_normal.sum().item())
        for b in sorted({0, B - 1}):
            want = ref.normals_image(depth[b, 0].cpu().numpy(), rp)
            assert nb.normal[b, 0].cpu().numpy().tobytes() == want.tobytes(), "the kernel and the float32 restatement disagree"
        out = {"shape": "%dx%d %s %dx%d %s" % (B, F, kind, cols, rows, im["depth_type"]), "batch": B, "frames": F, "image": kind,
               "radius": radius, "smooth": smooth, "pixels": pixels, "found_share": found / float(pixels), "cloud_rows": cloud_rows,
               "bytes": nbytes}
        results.append(out)
        if once:
            continue
        fns = {"normals": lambda: nb.run(ctx, p, depth, n_images=n_images), "rows": lambda: nb.run(ctx, p, depth, pose, n_images, cloud=dc),
               "copy": lambda: other.copy_(half), "cloud": lambda: dc.run(ctx, cp, depth, pose, n_images)}
        t = interleaved(fns, rounds)
        for k, (med, low) in t.items():
            out[k] = {"ms_median": med, "ms_min": low, "us_per_image": med * 1e3 / (B * F),
                      "GB_per_s": nbytes / (med * 1e-3) / 1e9 if k in ("normals", "copy") else None}
        out["rows_kernel_ms"] = t["rows"][0] - t["normals"][0]
        if with_torch and (radius, smooth) in TORCH_SETTINGS:
            flat = depth.view(B * F, rows, cols)
            scratch = torch.empty((B * F, rows, cols, 4), dtype=torch.float32, device=dev)
            rule = lambda: torch_rule(flat, im, radius, smooth, p.max_rel_diff, p.range_min, p.range_max, scratch)  # noqa: E731
            rule()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rule()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            mine, theirs = nb.normal.view(B * F, rows, cols, 4)[:4], scratch[:4]
            both = (mine[..., 3] > 0) & (theirs[..., 3] > 0)
            cos = (mine[..., :3].double() * theirs[..., :3].double()).sum(-1)[both].clamp(-1, 1)
            out["torch"] = {"ms": ms, "us_per_image": ms * 1e3 / (B * F), "same_pixels": bool(((mine[..., 3] > 0) == (theirs[..., 3] > 0)).all().item()),
                            "same_bytes": bool(torch.equal(mine, theirs)), "max_angle_rad": float(torch.acos(cos).max().item()) if both.any() else None}
            del scratch
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", default=["1x64", "64x16", "256x4"])
    ap.add_argument("--image", nargs="*", default=["vga", "kitti"], choices=sorted(IMAGES))
    ap.add_argument("--radius", nargs="*", type=int, default=[1, 2, 8])
    ap.add_argument("--smooth", nargs="*", type=int, default=[0, 1, 3])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_normals.py measures on the GPU"
    ctx = ops.Context(0)
    settings = [(r, s) for r in args.radius for s in args.smooth]
    results = []
    for kind in args.image:
        for shape in args.shape:
            B, F = (int(x) for x in shape.lower().split("x"))
            for r in bench(ctx, B, F, kind, settings, args.rounds, not args.no_torch, args.once):
                results.append(r)
                line = "%s r %d s %d (%.0f %% with a normal, %.1f MB):" % (r["shape"], r["radius"], r["smooth"], 100 * r["found_share"], r["bytes"] / 1e6)
                for k in ("normals", "rows", "copy", "cloud"):
                    if k in r:
                        line += "  %s %.4f ms (min %.4f, %.2f us an image)" % (k, r[k]["ms_median"], r[k]["ms_min"], r[k]["us_per_image"])
                        line += ", %.0f GB/s" % r[k]["GB_per_s"] if r[k]["GB_per_s"] else ""
                print(line, flush=True)
                if "copy" in r:
                    print("    the call takes %.2f x the copy of its bytes and %.2f x the cloud call; the rows kernel adds %.4f ms" % (
                        r["normals"]["ms_median"] / r["copy"]["ms_median"], r["normals"]["ms_median"] / r["cloud"]["ms_median"], r["rows_kernel_ms"]),
                        flush=True)
                if "torch" in r:
                    t = r["torch"]
                    print("    torch ops: %.2f ms (%.1f us an image), %.0f x the call; same pixels %s, same bytes %s, largest angle %s rad" % (
                        t["ms"], t["us_per_image"], t["ms"] / r["normals"]["ms_median"], t["same_pixels"], t["same_bytes"], t["max_angle_rad"]),
                        flush=True)
            torch.cuda.empty_cache()
    ctx.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
