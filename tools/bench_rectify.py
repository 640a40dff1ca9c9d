"""Image rectifier throughput (prs_rectify_batch_run): B EuRoC-shaped stereo pairs (752 x 480, 8-bit, bilinear) resident in HBM, and B
640 x 480 uint16 depth images in nearest mode.
usage: python tools/bench_rectify.py [B ...] [--variant a|b|all] [--rounds N] [--json FILE] [--no-host]
  Inputs are synthetic.stereo_images pairs replicated over the batch (left block, then right block: ops.RectifyBatch's stereo layout)
  and the two maps of ops.stereo_rectification for a seeded EuRoC-like calibration.  Per batch size, in one process:
    rectify    ms per launch and bytes per second of src + dst (1 B read and 1 B written per pixel), for every selected kernel variant
               in interleaved rounds (median and minimum over the rounds); the variants' outputs are compared byte for byte
    copy       a plain device-to-device copy of the same bytes: the ceiling the kernel is judged against
    extract    prs_extract_features_batch on the rectified images: the stage the kernel feeds
    host       the route it replaces: .cpu(), the numpy restatement (tests/rectify_ref.py) on one image scaled to the batch, the upload
  --variant: tap fetch (a) per-lane loads from global memory, (b) the tile's source footprint staged in LDS (what ships for 8-bit
  bilinear; nearest always fetches as (a)), selected through PRS_RECTIFY_VARIANT (0: (a)), which the library reads per launch.
  Batch sizes default to 1 256 4096."""
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

from srrg2_proslam_amd import configs, ops, synthetic as syn  # noqa: E402

K0 = np.array([[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]])  # EuRoC cam0
D0 = np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0])
K_TUM = np.array([[517.3, 0.0, 318.6], [0.0, 516.5, 255.3], [0.0, 0.0, 1.0]])  # TUM freiburg1
D_TUM = np.array([0.2624, -0.9531, -0.0054, 0.0026, 1.1633])
VARIANTS = {"a": 0, "b": 1}


def seeded_stereo_maps(seed=0):
    """an EuRoC-like calibration: cam0's numbers jittered, 2-3 degrees between the cameras, 11 cm of baseline with offsets in y and z"""
    rng = np.random.default_rng(seed)
    Kl = K0 + np.array([[rng.normal(0, 2), 0, rng.normal(0, 3)], [0, rng.normal(0, 2), rng.normal(0, 3)], [0, 0, 0]])
    Kr = K0 + np.array([[rng.normal(0, 2), 0, rng.normal(0, 3)], [0, rng.normal(0, 2), rng.normal(0, 3)], [0, 0, 0]])
    ang = np.deg2rad(rng.uniform(2.0, 3.0))
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R_rl = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    t_rl = np.array([0.11, rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)])
    return ops.stereo_rectification(Kl, D0 * (1 + rng.normal(0, 0.05, 5)), Kr, D0 * (1 + rng.normal(0, 0.05, 5)), R_rl, t_rl, (752, 480))


def _window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _iters(fn, seconds=0.25):
    """warm up, then the number of launches that fills `seconds`"""
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


def with_variant(code, fn):
    def run():
        os.environ["PRS_RECTIFY_VARIANT"] = str(code)
        fn()
    return run


def bench_stereo(ctx, pairs, variants, rounds, host):
    import rectify_ref as ref
    cfg = configs.EUROC
    base = [syn.stereo_images(np.random.default_rng(syn.seed_for(7, k)), cfg)[:2] for k in range(4)]
    dev = torch.device("cuda", 0)
    lefts = torch.from_numpy(np.stack([p[0] for p in base])).to(dev)
    rights = torch.from_numpy(np.stack([p[1] for p in base])).to(dev)
    idx = torch.arange(pairs, device=dev) % len(base)
    src = torch.cat([lefts[idx], rights[idx]])  # left block, right block
    ml, mr, _ = seeded_stereo_maps()
    B = 2 * pairs
    rb = ops.RectifyBatch(ctx, ops.rectify_params(), [ml, mr], B, src.shape[1:], stereo=True)
    nbytes = 2 * src.numel()
    outs = {}
    for name, code in variants.items():
        with_variant(code, lambda: rb.run(src))()
        torch.cuda.synchronize()
        assert int(rb.status.abs().max().item()) == 0
        outs[name] = rb.dst[:: max(B // 8, 1)].cpu().numpy().copy()
    first = next(iter(outs.values()))
    assert all(np.array_equal(first, o) for o in outs.values()), "the variants disagree"
    want = ref.rectify(base[0][0], ml)[0]
    assert np.array_equal(first[0], want), "the kernel and the float32 restatement disagree"
    fns = {name: with_variant(code, lambda: rb.run(src)) for name, code in variants.items()}
    copy_dst = torch.empty_like(src)
    fns["copy"] = lambda: copy_dst.copy_(src)
    t = interleaved(fns, rounds)
    del copy_dst
    os.environ.pop("PRS_RECTIFY_VARIANT", None)
    rb.run(src)
    ep = ops.extractor_params()
    kp = torch.zeros((B, 2048, 2), dtype=torch.float32, device=dev)
    desc = torch.zeros((B, 2048, 32), dtype=torch.uint8, device=dev)
    n, st = torch.zeros((B,), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev)
    t.update(interleaved({"extract": lambda: ops.extract_features_batch(ctx, ep, rb.dst, kp, desc, n, st)}, rounds))
    assert int(st.min().item()) >= 0
    out = {"shape": "stereo 752x480 u8 bilinear", "pairs": pairs, "images": B, "bytes": nbytes,
           "features_per_image": float(n.float().mean().item()), "border_share": float(rb.n_border.float().mean().item()) / (480 * 752)}
    for k, (med, low) in t.items():
        out[k] = {"ms_median": med, "ms_min": low, "GB_per_s": nbytes / (med * 1e-3) / 1e9 if k != "extract" else None}
    if host:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = src.cpu()
        t1 = time.perf_counter()
        one = h[0].numpy()
        ref.rectify(one, ml)
        t2 = time.perf_counter()
        ref.rectify(one, ml)
        t3 = time.perf_counter()
        h.to(dev)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        out["host"] = {"download_ms": (t1 - t0) * 1e3, "numpy_ms_per_image": (t3 - t2) * 1e3, "numpy_ms_scaled": (t3 - t2) * 1e3 * B,
                       "upload_ms": (t4 - t3) * 1e3, "total_ms": ((t1 - t0) + (t3 - t2) * B + (t4 - t3)) * 1e3}
    return out


def bench_depth(ctx, B, variants, rounds):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    base = torch.from_numpy(rng.integers(400, 6000, (4, 480, 640)).astype(np.int16)).to(dev)  # (no uint16 gather in torch)
    src = base[torch.arange(B, device=dev) % 4].view(torch.uint16)
    m = ops.rectify_map(K_TUM, D_TUM, None, np.array([[525.0, 0.0, 319.5], [0.0, 525.0, 239.5], [0.0, 0.0, 1.0]]))
    rb = ops.RectifyBatch(ctx, ops.rectify_params("u16"), [m], B, (480, 640))
    nbytes = 2 * src.numel() * 2
    fns = {"a": with_variant(0, lambda: rb.run(src))}  # nearest is never staged
    copy_dst = torch.empty_like(src)
    fns["copy"] = lambda: copy_dst.view(torch.int16).copy_(src.view(torch.int16))
    t = interleaved(fns, rounds)
    os.environ.pop("PRS_RECTIFY_VARIANT", None)
    assert int(rb.status.abs().max().item()) == 0
    out = {"shape": "depth 640x480 u16 nearest", "images": B, "bytes": nbytes,
           "border_share": float(rb.n_border.float().mean().item()) / (480 * 640)}
    for k, (med, low) in t.items():
        out[k] = {"ms_median": med, "ms_min": low, "GB_per_s": nbytes / (med * 1e-3) / 1e9}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", nargs="*", type=int, default=[1, 256, 4096])
    ap.add_argument("--variant", choices=["a", "b", "all"], default="all")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    variants = {k: c for k, c in VARIANTS.items() if args.variant in (k, "all")}
    assert torch.cuda.is_available(), "bench_rectify.py measures on the GPU"
    ctx = ops.Context(0)
    results = []
    for B in args.batch:
        for r in (bench_stereo(ctx, B, variants, args.rounds, not args.no_host), bench_depth(ctx, B, variants, args.rounds)):
            results.append(r)
            line = "%s B=%d (%.1f MB src + dst, %.2f %% border):" % (r["shape"], r.get("pairs", r["images"]), r["bytes"] / 1e6, 100 * r["border_share"])
            for k, v in r.items():
                if isinstance(v, dict) and "ms_median" in v:
                    line += "  %s %.4f ms (min %.4f)" % (k, v["ms_median"], v["ms_min"]) + (", %.0f GB/s" % v["GB_per_s"] if v["GB_per_s"] else "")
            print(line, flush=True)
            if "extract" in r:
                for k in variants:
                    print("    %s: %.1f %% of the copy ceiling, %.1f %% of the extractor's time, %.1f %% of rectify + extract" % (
                        k, 100 * r["copy"]["ms_median"] / r[k]["ms_median"], 100 * r[k]["ms_median"] / r["extract"]["ms_median"],
                        100 * r[k]["ms_median"] / (r[k]["ms_median"] + r["extract"]["ms_median"])), flush=True)
            if "host" in r:
                h = r["host"]
                print("    host route: download %.1f ms + numpy %.1f ms an image x %d = %.0f ms + upload %.1f ms = %.0f ms" % (
                    h["download_ms"], h["numpy_ms_per_image"], r["images"], h["numpy_ms_scaled"], h["upload_ms"], h["total_ms"]), flush=True)
            torch.cuda.empty_cache()
    ctx.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
