"""Dense aligner throughput (prs_dense_align_batch_run): B pairs of a rendered model view and a live 640 x 480 16-bit depth frame,
everything resident in HBM.
usage: python tools/bench_dense_align.py [B ...] [--rounds N] [--json FILE] [--once] [--linearise-only]
  The frames are those of tools/bench_tsdf.py: seeded 16-bit depth frames of a rolling surface between 1.5 and 3.5 m, seen along a
  gentle walk, V of them fused into a cube of 4 m of 128^3 voxels in front of the first camera.  Model view b is the raycast of that
  volume from the pose of frame b mod V (ONE raycast call of B views), live image b is frame b mod V itself, and the estimate starts
  a centimetre and a few milliradians off.  Per batch size, in one process, timed with events on the stream in interleaved rounds
  (median and minimum over the rounds):
    step4, step2, step1   one call of 5 iterations on every fourth, every second and every pixel: per call and per linearisation
    schedule              the default schedule configs.DENSE_ALIGN["schedule"] (19 linearisations in three calls)
    copy                  (a) a device-to-device copy of as many bytes as ONE linearisation at step 1 reads (22 a pixel: 2 live,
                          4 + 16 model), so it reads 22 and writes 22
    raycast               (b) the raycast call that produced the B model views
    torch                 (c) one linearisation at step 1 written in torch ops (the same association, gates and weights; H = G^T W G),
                          64 pairs at a time
  Batch sizes default to 1 64 256.  Pair 0 at step 4 is compared with the numpy restatement byte for byte.  --once: one call a
  shape and that comparison, no timing (for a profiler).  --linearise-only: step 1 with linearize_only alone (what the choice of
  PRS_DENSE_ALIGN_SAMPLES_PER_THREAD was timed with)."""
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
EXTENT, N, V = 4.0, 128, 4
ITERATIONS = 5


def start_estimate(B, dev):
    c, s = np.cos(0.004), np.sin(0.004)
    X0 = np.array([[c, 0, s, 0.01], [0, 1, 0, -0.005], [-s, 0, c, 0.008], [0, 0, 0, 1]], np.float32)
    return X0, torch.from_numpy(X0.reshape(1, 16)).to(dev).repeat(B, 1).contiguous()


def torch_linearisation(p, X, model_depth, model_normal, live):
    """one linearisation at step 1 in torch ops -> (H [B, 6, 6], b [B, 6]) in the camera frame (float32, torch's own order)"""
    B, rows, cols = live.shape
    dev = live.device
    v, u = torch.meshgrid(torch.arange(rows, device=dev, dtype=torch.float32), torch.arange(cols, device=dev, dtype=torch.float32), indexing="ij")
    d = live.view(torch.int16).to(torch.float32) * p.depth_scaling_factor_to_meters
    ok = (d >= p.range_min) & (d <= p.range_max)
    pt = torch.stack([(u - p.cx) / p.fx * d, (v - p.cy) / p.fy * d, d], -1)                 # [B, rows, cols, 3]
    T = X.view(B, 4, 4)
    y = torch.einsum("bij,bvuj->bvui", T[:, :3, :3], pt)
    m = y + T[:, None, None, :3, 3]
    ok &= m[..., 2] > 0
    uf = torch.floor(m[..., 0] / m[..., 2] * p.fx + p.cx + 0.5)
    vf = torch.floor(m[..., 1] / m[..., 2] * p.fy + p.cy + 0.5)
    ok &= (uf >= 0) & (uf < cols) & (vf >= 0) & (vf < rows)
    index = (torch.where(ok, vf, torch.zeros_like(vf)) * cols + torch.where(ok, uf, torch.zeros_like(uf))).to(torch.int64).view(B, -1)
    dm = torch.gather(model_depth.reshape(B, -1), 1, index).view(B, rows, cols)
    nr = torch.gather(model_normal.reshape(B, -1, 4), 1, index[..., None].expand(-1, -1, 4)).view(B, rows, cols, 4)
    ok &= (dm > 0) & (nr[..., 3] > 0)
    um, vm = (index % cols).view(B, rows, cols).to(torch.float32), (index // cols).view(B, rows, cols).to(torch.float32)
    f = torch.stack([(um - p.cx) / p.fx * dm, (vm - p.cy) / p.fy * dm, dm], -1)
    e = m - f
    n = nr[..., :3]
    r = (n * e).sum(-1)
    chi = r * r
    ok &= ((e * e).sum(-1) <= p.max_distance * p.max_distance) & torch.isfinite(chi)
    w = torch.where(chi <= p.chi_threshold, torch.ones_like(chi), 1.0 / chi) * ok
    g = torch.cat([n, torch.cross(y, n, dim=-1)], -1).view(B, -1, 6)
    gw = g * torch.nan_to_num(w).view(B, -1, 1)
    return gw.transpose(1, 2) @ g, (gw * torch.nan_to_num(r).view(B, -1, 1)).sum(1)


def bench(ctx, B, rounds, once, linearise_only):
    import dense_align_ref as ref
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    frames_np = seeded_depth(rng, ROWS, COLS, "u16")
    frames = torch.from_numpy(frames_np.view(np.int16)).to(dev).view(torch.uint16).view(1, V, ROWS, COLS)
    pose_np = seeded_poses(rng, V)
    pose = torch.from_numpy(pose_np).to(dev).view(1, V, 16)
    vs = EXTENT / N
    vb = ops.TsdfVolumeBatch(1, N, N, N, V, ROWS, COLS)
    vb.origin.copy_(torch.tensor([[-EXTENT / 2, -EXTENT / 2, 0.5, 0.0]], dtype=torch.float32))
    vb.integrate(ctx, ops.tsdf_params(CAMERA, voxel_size=vs, truncation=4 * vs, scale=SCALE), frames, pose)
    rb = ops.TsdfRaycastBatch(ctx, vb, B, ROWS, COLS)
    rp = ops.tsdf_raycast_params(CAMERA, voxel_size=vs, step=vs)
    view_index = (torch.arange(B, device=dev, dtype=torch.int32) % V).view(1, B).contiguous()
    depth, normal, n_hit = rb.run(rp, pose, view_index=view_index)
    model_depth, model_normal = depth.view(B, ROWS, COLS), normal.view(B, ROWS, COLS, 4)
    live = frames.view(V, ROWS, COLS).view(torch.int16)[torch.arange(B, device=dev) % V].view(torch.uint16)  # (no uint16 gather in torch)
    X0_np, X0 = start_estimate(B, dev)
    ab = ops.DenseAlignBatch(ctx, B, ROWS, COLS)
    p = ops.dense_align_params(CAMERA, "u16", SCALE, max_iterations=ITERATIONS)

    def call(step, q=p):
        ab.X.copy_(X0)
        return ab.run(q, model_depth, model_normal, live, None, step)

    def schedule():
        ab.X.copy_(X0)
        return ab.align(p, model_depth, model_normal, live)

    call(4)
    torch.cuda.synchronize()
    md, mn = model_depth[0].cpu().numpy(), model_normal[0].cpu().numpy()
    Xr, res, _ = ref.align(ref.params(CAMERA, "u16", SCALE, max_iterations=ITERATIONS), X0_np, md, mn, frames_np[0], None, 4)
    got = ab.results()[0]
    assert ab.X[0].cpu().numpy().tobytes() == Xr.tobytes() and got["H"].tobytes() == res["H"].tobytes() and \
        int(got["num_inliers"]) == res["num_inliers"], "the kernel and the float32 restatement disagree"
    schedule()
    torch.cuda.synchronize()
    last = ab.results()
    pixels = B * ROWS * COLS
    out = {"shape": "%d vga pairs" % B, "batch": B, "pixels": pixels, "hit_share": int(n_hit.sum().item()) / float(pixels),
           "inlier_share": float(last["num_inliers"].sum()) / pixels, "steps_taken": int(last["steps_taken"].min()),
           "read_bytes": pixels * 22}
    if once:
        return out
    lin = ops.dense_align_params(CAMERA, "u16", SCALE, max_iterations=0, linearize_only=1)
    if linearise_only:
        t = interleaved({"linearise": lambda: call(1, lin)}, rounds)
        out["linearise"] = {"ms_median": t["linearise"][0], "ms_min": t["linearise"][1]}
        return out
    read = torch.empty((pixels * 22,), dtype=torch.uint8, device=dev)
    other = torch.empty_like(read)

    def in_torch():  # 64 pairs at a time: its intermediates take about 150 bytes a pixel
        for b0 in range(0, B, 64):
            b1 = min(b0 + 64, B)
            torch_linearisation(p, X0[b0:b1], model_depth[b0:b1], model_normal[b0:b1], live[b0:b1])
    fns = {"step4": lambda: call(4), "step2": lambda: call(2), "step1": lambda: call(1), "schedule": schedule,
           "linearise": lambda: call(1, lin), "copy": lambda: other.copy_(read),
           "raycast": lambda: rb.run(rp, pose, view_index=view_index), "torch": in_torch}
    t = interleaved(fns, rounds)
    n_lin = {"step4": ITERATIONS, "step2": ITERATIONS, "step1": ITERATIONS, "linearise": 1,
             "schedule": sum(i for _, i in configs.DENSE_ALIGN["schedule"])}
    for k, (med, low) in t.items():
        out[k] = {"ms_median": med, "ms_min": low}
        if k in n_lin:
            out[k]["ms_per_linearisation"] = med / n_lin[k]
    out["copy"]["GB_per_s"] = out["read_bytes"] / (t["copy"][0] * 1e-3) / 1e9
    out["linearise"]["Msamples_per_s"] = pixels / (t["linearise"][0] * 1e-3) / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", nargs="*", type=int, default=[1, 64, 256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--linearise-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dense_align.py measures on the GPU"
    ctx = ops.Context(0)
    results = []
    for B in args.batch:
        r = bench(ctx, B, args.rounds, args.once, args.linearise_only)
        results.append(r)
        line = "%s (%.1f %% of the model's pixels hit, %.1f %% of the samples inliers after the schedule, %d steps):" % (
            r["shape"], 100 * r["hit_share"], 100 * r["inlier_share"], r["steps_taken"])
        for k in ("step4", "step2", "step1", "schedule", "linearise", "copy", "raycast", "torch"):
            if k in r:
                line += "  %s %.4f ms (min %.4f%s)" % (k, r[k]["ms_median"], r[k]["ms_min"],
                                                       ", %.4f a linearisation" % r[k]["ms_per_linearisation"] if "ms_per_linearisation" in r[k] else "")
        print(line, flush=True)
        if "copy" in r:
            print("    one linearisation at step 1: %.0f Msamples/s, %.2f x the copy of what it reads, %.3f x the raycast call%s" % (
                r["linearise"]["Msamples_per_s"], r["linearise"]["ms_median"] / r["copy"]["ms_median"],
                r["linearise"]["ms_median"] / r["raycast"]["ms_median"],
                ", %.3f x the torch ops" % (r["linearise"]["ms_median"] / r["torch"]["ms_median"]) if "torch" in r else ""), flush=True)
        torch.cuda.empty_cache()
    ctx.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
