"""RGB-D preprocessor throughput (prs_extract_features_batch + prs_depth_measurements_batch): B ICL frames resident in HBM
usage: python tools/bench_rgbd.py [B ...] [--config icl|tum|both]
  the three ICL frames of tests/golden/ref_icl.npz (640 x 480, uint16 millimetre depth) replicated over the batch, extracted with
  the configuration's "rgbd" group (FAST 5, 3x3 detectors; icl 500 / tum 1000 keypoints, depth scale 0.001).  Reports extraction
  alone against extraction plus the depth stage, images per second, and the depth stage's time per launch with its algorithmic
  bytes per second: per feature the keypoint (8 B) and the depth element (2 B), per kept feature (u, v, d, 0) (16 B), the
  descriptor read and written (64 B) and the intensity read and written (8 B).  Batch sizes default to 1 16 256 1024 4096."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from srrg2_proslam_amd import configs, ops  # noqa: E402


def _time(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def run(B, config="icl", iters=10):
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_icl.npz"))
    gray, mm = z["gray"], z["depth_mm"]
    cfg = configs.get(config)
    ep, dp = ops.rgbd_params(cfg)
    dev = torch.device("cuda", 0)
    idx = torch.arange(B, device=dev) % len(gray)
    fr = ops.RGBDFrames(0, B, gray.shape[1], gray.shape[2], 2048)
    fr.images.copy_(torch.from_numpy(gray).to(dev)[idx])
    fr.depth.view(torch.int16).copy_(torch.from_numpy(mm.view(np.int16)).to(dev)[idx])  # (no uint16 gather in torch)
    ctx = ops.Context(0)
    ctx.use_torch_stream()
    ms_extract = _time(lambda: fr.extract(ctx, ep), iters)
    ms_both = _time(lambda: fr.run(ctx, ep, dp), iters)
    ms_depth = _time(lambda: fr.measure(ctx, dp), iters * 10)  # the depth stage alone, on the extractor's last outputs
    fr.run(ctx, ep, dp)
    torch.cuda.synchronize()
    assert int(fr.status.min().item()) >= 0, "an image failed: status %d" % int(fr.status.min().item())
    n = fr.n_features.long().sum().item()
    kept = fr.n_fixed.long().sum().item()
    nbytes = n * (8 + 2) + kept * (16 + 64 + 8) + B * 16
    ctx.close()
    return {"config": config, "images_per_launch": B, "features_per_image": n / B, "kept_per_image": kept / B,
            "ms_extract": ms_extract, "ms_extract_depth": ms_both, "us_depth": ms_depth * 1e3, "images_per_s": B / (ms_both * 1e-3),
            "depth_share": ms_depth / ms_extract, "depth_GB_per_s": nbytes / (ms_depth * 1e-3) / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", nargs="*", type=int, default=[1, 16, 256, 1024, 4096])
    ap.add_argument("--config", choices=["icl", "tum", "both"], default="both")
    args = ap.parse_args()
    for config in (["icl", "tum"] if args.config == "both" else [args.config]):
        for B in args.batch:
            r = run(B, config)
            print("%s B=%d %.0f features/image (%.0f with depth): extract %.3f ms, extract + depth %.3f ms (%.0f images/s); depth stage "
                  "%.1f us/launch (%.1f %% of extraction), %.0f GB/s algorithmic" % (
                      r["config"], B, r["features_per_image"], r["kept_per_image"], r["ms_extract"], r["ms_extract_depth"], r["images_per_s"],
                      r["us_depth"], 100 * r["depth_share"], r["depth_GB_per_s"]))


if __name__ == "__main__":
    main()
