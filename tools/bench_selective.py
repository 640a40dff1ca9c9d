"""selective extractor throughput (GFTT + ORB, prs_extract_features_selective_batch): B KITTI frames resident in HBM
usage: python tools/bench_selective.py [B ...] [--mode seeding|tracking]
  the fourteen KITTI frames of tests/golden/ref_kitti.npz (1241 x 376) replicated over the batch; the reference's gtest settings
  (target_bin_width_pixels 10).  seeding: 100 keypoints in the whole image; tracking: 1000 keypoints around 94 projections of
  radius 50 per image, plus seeding in the rest of the image.  Batch sizes default to 1 16 256 4096."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from srrg2_proslam_amd import ops  # noqa: E402


def run(B, mode="tracking", iters=5):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_kitti.npz"))
    uniq = [im for key in ("city_left", "city_right", "highway_left", "highway_right") for im in z[key]]
    dev = torch.device("cuda", 0)
    stage = torch.from_numpy(np.stack(uniq)).to(dev)
    img = stage[torch.arange(B, device=dev) % len(uniq)].contiguous()
    rows, cols = int(img.shape[1]), int(img.shape[2])
    stride = 4096
    kp = torch.zeros((B, stride, 2), dtype=torch.float32, device=dev)
    desc = torch.zeros((B, stride, 32), dtype=torch.uint8, device=dev)
    n = torch.zeros((B,), dtype=torch.int32, device=dev)
    st = torch.zeros((B,), dtype=torch.int32, device=dev)
    ctx = ops.Context(0)
    ctx.use_torch_stream()
    kw = {}
    if mode == "tracking":
        rng = np.random.default_rng(0)
        proj = np.stack([rng.uniform(40, cols - 40, 94), rng.uniform(40, rows - 40, 94)], 1).astype(np.float32)
        kw = dict(projections=torch.from_numpy(np.broadcast_to(proj, (B, 94, 2)).copy()).to(dev),
                  n_projections=torch.full((B,), 94, dtype=torch.int32, device=dev), radius=torch.full((B,), 50, dtype=torch.int32, device=dev))
        p = ops.selective_extractor_params("GFTT", "ORB-256", 1000, 10)
    else:
        p = ops.selective_extractor_params("GFTT", "ORB-256", 100, 10)
    for _ in range(2):
        ops.extract_features_selective_batch(ctx, p, img, kp, desc, n, st, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.extract_features_selective_batch(ctx, p, img, kp, desc, n, st, **kw)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    assert int(st.min().item()) >= 0, "an image failed: status %d" % int(st.min().item())
    nf = n.float().mean().item()
    ctx.close()
    return {"mode": mode, "images_per_launch": B, "image": "%dx%d" % (cols, rows), "features_per_image": nf, "ms_per_launch": ms,
            "images_per_s": B / (ms * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", nargs="*", type=int, default=[1, 16, 256, 4096])
    ap.add_argument("--mode", choices=["seeding", "tracking"], default="tracking")
    args = ap.parse_args()
    for B in args.batch:
        r = run(B, args.mode)
        print("%s B=%d images %s, %.0f features/image: %.3f ms/launch, %.0f images/s" % (
            r["mode"], B, r["image"], r["features_per_image"], r["ms_per_launch"], r["images_per_s"]))


if __name__ == "__main__":
    main()
