"""TSDF mesh throughput (prs_tsdf_mesh_batch_run): the volumes tools/bench_tsdf.py fuses -- B sequences of F seeded VGA depth frames
into one N x N x N volume a sequence, a cube of 4 m -- turned into an indexed quad mesh a sequence.
usage: python tools/bench_tsdf_mesh.py [BxFxN ...] [--rounds N] [--json FILE] [--once] [--kernels]
  Per shape, in one process, timed with events on the stream in interleaved rounds (median and minimum over the rounds):
    mesh     ms per call with vertex, normal, quad, cube and edge (four launches)
    count    the count-only call (two launches: count and scan)
    surface  prs_tsdf_surface_batch_run with xyz, normal and cell on the same volumes: the nearest stage that existed before
    copy     a device-to-device copy of the volume's bytes (8 read and 8 written a voxel): the floor of one pass over the volume
  Shapes default to 1x64x256 64x16x128 256x4x64, F being the frames fused beforehand.  The mesh of the first and the last sequence
  of a volume of 64^3 is compared with the numpy restatement byte for byte.  --once: ten mesh calls and that comparison, no timing
  (for a profiler).  --kernels: runs itself with --once under `rocprofv3 --kernel-trace --stats` in a child process per shape and
  adds the mean time of each of the call's four kernels."""
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

from srrg2_proslam_amd import configs, ops  # noqa: E402
from bench_depth_cloud import interleaved, seeded_poses  # noqa: E402
from bench_depth_normals import seeded_depth  # noqa: E402
from bench_tsdf import CAMERA, COLS, EXTENT, ROWS, SCALE  # noqa: E402

KERNELS = ("tsdf_mesh_count_kernel", "tsdf_mesh_scan_kernel", "tsdf_mesh_vertices_kernel", "tsdf_mesh_quads_kernel")


def bench(ctx, B, F, N, rounds, once):
    import tsdf_mesh_ref as ref
    import tsdf_ref
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)  # the seed, depth and walk of tools/bench_tsdf.py
    base = torch.from_numpy(seeded_depth(rng, ROWS, COLS, "u16").view(np.int16)).to(dev)
    depth = base[torch.arange(B * F, device=dev) % 4].view(torch.uint16).view(B, F, ROWS, COLS)
    pose = torch.from_numpy(seeded_poses(rng, F)).to(dev).repeat(B, 1, 1).contiguous()
    n_images = torch.full((B,), F, dtype=torch.int32, device=dev)
    vs = EXTENT / N
    kw = dict(voxel_size=vs, truncation=4 * vs, max_weight=configs.TSDF["max_weight"], min_weight=configs.TSDF["min_weight"],
              range_min=configs.TSDF["range_min"], range_max=configs.TSDF["range_max"], scale=SCALE)
    p, rp = ops.tsdf_params(CAMERA, **kw), tsdf_ref.params(CAMERA, **kw)
    voxels = N * N * N
    cap = min(voxels // 2, 8 << 20)
    vb = ops.TsdfVolumeBatch(B, N, N, N, F, ROWS, COLS, out_stride=cap)
    origin_np = np.array([-EXTENT / 2, -EXTENT / 2, 0.5, 0.0], np.float32)
    vb.origin.copy_(torch.from_numpy(np.tile(origin_np, (B, 1))))
    vb.integrate(ctx, p, depth, pose, n_images)
    del depth
    mb = ops.TsdfMeshBatch(vb, cap, cap)
    mb.run(ctx, p)
    vb.surface(ctx, p)
    torch.cuda.synchronize()
    assert int(vb.status.abs().max().item()) == 0
    out = {"shape": "%dx%d vga u16 into %d^3" % (B, F, N), "batch": B, "frames": F, "n": N, "voxels": B * voxels,
           "vertices": int(mb.n_vertices_total.sum().item()), "quads": int(mb.n_quads_total.sum().item()),
           "crossings": int(vb.n_total.sum().item()), "capacity_hit": bool((mb.status != 0).any().item() or (vb.surface_status != 0).any().item()),
           "volume_bytes": B * voxels * 8, "workspace_bytes": int(mb.workspace.numel())}
    if N <= 64:
        for b in sorted({0, B - 1}):
            want = ref.mesh(vb.volume[b].cpu().numpy(), rp, origin_np, cap, cap)
            nv, nq = want["n_vertices"], want["n_quads"]
            assert (int(mb.n_vertices[b].item()), int(mb.n_quads[b].item())) == (nv, nq), "the counts and the restatement disagree"
            for name, n in (("vertex", nv), ("normal", nv), ("cube", nv), ("quad", nq), ("edge", nq)):
                assert getattr(mb, name)[b, :n].cpu().numpy().tobytes() == want[name][:n].tobytes(), "%s and the restatement disagree" % name
        out["checked"] = True
    if once:
        for _ in range(10):
            mb.run(ctx, p)
        torch.cuda.synchronize()
        return out
    half, other = torch.empty_like(vb.volume), torch.empty_like(vb.volume)
    fns = {"mesh": lambda: mb.run(ctx, p), "count": lambda: mb.count(ctx, p), "surface": lambda: vb.surface(ctx, p),
           "copy": lambda: other.copy_(half)}
    for k, (med, low) in interleaved(fns, rounds).items():
        out[k] = {"ms_median": med, "ms_min": low}
    out["copy"]["GB_per_s"] = 2 * out["volume_bytes"] / (out["copy"]["ms_median"] * 1e-3) / 1e9
    return out


def kernel_times(shape):
    """{kernel: mean microseconds} of the mesh call's kernels from a kernel trace of a child process that runs this tool with --once"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), shape,
               "--once"]
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            raise RuntimeError("the profiled child failed:\n" + done.stdout[-2000:] + done.stderr[-2000:])
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in KERNELS:
                    if k in row.get("Name", ""):
                        out[k] = {"us_mean": float(row["AverageNs"]) / 1e3, "calls": int(row["Calls"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", default=["1x64x256", "64x16x128", "256x4x64"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tsdf_mesh.py measures on the GPU"
    ctx = ops.Context(0)
    results = []
    for shape in args.shape:
        B, F, N = (int(x) for x in shape.lower().split("x"))
        r = bench(ctx, B, F, N, args.rounds, args.once)
        results.append(r)
        line = "%s (%d vertices, %d quads, %d crossings%s, volume %.1f MB, workspace %.1f MB):" % (
            r["shape"], r["vertices"], r["quads"], r["crossings"], ", CAPACITY" if r["capacity_hit"] else "", r["volume_bytes"] / 1e6,
            r["workspace_bytes"] / 1e6)
        for k in ("mesh", "count", "surface", "copy"):
            if k in r:
                line += "  %s %.4f ms (min %.4f)" % (k, r[k]["ms_median"], r[k]["ms_min"])
        print(line, flush=True)
        if "mesh" in r:
            print("    mesh takes %.2f x the surface call and %.2f x the copy of the volume (%.0f GB/s); count only %.2f x the copy" % (
                r["mesh"]["ms_median"] / r["surface"]["ms_median"], r["mesh"]["ms_median"] / r["copy"]["ms_median"], r["copy"]["GB_per_s"],
                r["count"]["ms_median"] / r["copy"]["ms_median"]), flush=True)
        torch.cuda.empty_cache()
        if args.kernels and not args.once:
            r["kernels"] = kernel_times(shape)
            print("    " + ", ".join("%s %.1f us" % (k.replace("tsdf_mesh_", "").replace("_kernel", ""), v["us_mean"])
                                     for k, v in r["kernels"].items()), flush=True)
    ctx.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
