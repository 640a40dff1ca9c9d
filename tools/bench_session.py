#!/usr/bin/env python3
"""The closed tracking loop of tools/bench_tracking.py with the local-map manager on the device (ops.SessionBatch) in place of the
host's split schedule: every sequence decides its own splits from its own pose, grows its pose graph and resets its map, with no
device-to-host read per frame.  Per frame:
   stereo matcher -> scene clipper at the session's prediction -> projective finder + GN aligner -> session step -> merger
The step's time is also measured beside the launches it replaces (pose_compose, the copy of the previous pose, motion_predict, the
flag copy and the two copies into the merger's pose arrays), alternating in one run, with device events, after warm-up.

    python tools/bench_session.py [--batches 1,256,4096] [--frames 60] [--unique 5] [--keypoints 2000]
prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def step_against_replaced(ctx, B, reps=200, warmup=20, device=0):
    """(microseconds per session step, microseconds per set of the launches it replaces), both at standstill (no split)"""
    import torch
    from srrg2_proslam_amd import configs, ops
    dev = torch.device("cuda", device)
    maps, frames = ops.MapBatch(device, B, 64, 1, 4, 1, 1), ops.AlignFrames(device, B, 1, 1)
    graphs = ops.PoseGraphBatch(device, B, 2, 2, envelope_blocks=3)
    sess = ops.SessionBatch(device, maps, frames, graphs, reps + warmup + 1)
    params = ops.session_params(configs.get("kitti")["split"])
    eye = torch.eye(4, dtype=torch.float32, device=dev).reshape(1, 16).repeat(B, 1).contiguous()
    frames.X.copy_(eye)
    frames.result.view(torch.int32)[:, ops.AlignResult.status.offset // 4] = 1
    pose, prev, pred = eye.clone(), eye.clone(), eye.clone()
    flags = torch.zeros((B,), dtype=torch.int32, device=dev)
    warn_off = ops.AlignResult.warnings.offset

    def replaced():
        prev.copy_(pose, non_blocking=True)
        ops.pose_compose_batch(ctx, pred, frames.X, pose)
        flags.copy_(frames.result[:, warn_off: warn_off + 4].contiguous().view(torch.int32).view(B), non_blocking=True)
        maps.measurement_in_world.copy_(pose.view(B, 4, 4), non_blocking=True)
        maps.measurement_in_scene.copy_(pose.view(B, 4, 4), non_blocking=True)
        ops.motion_predict_batch(ctx, prev, pose, pred)

    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for _ in range(warmup):
        sess.step(ctx, params)
        replaced()
    torch.cuda.synchronize()
    for i in range(reps):
        ev[i][0].record()
        sess.step(ctx, params)
        ev[i][1].record()
        replaced()
        ev[i][2].record()
    torch.cuda.synchronize()
    assert int(sess.status.abs().max().item()) == 0
    a = np.median([e[0].elapsed_time(e[1]) for e in ev]) * 1e3
    b = np.median([e[1].elapsed_time(e[2]) for e in ev]) * 1e3
    return float(a), float(b)


def run(batch=4096, frames=60, unique=5, keypoints=2000, cap=6144, prior_info=1.0, max_fixed=1024, device=0, seqs=None):
    import torch
    import bench_tracking as bt
    from bench_merge import merger_params
    from srrg2_proslam_amd import configs, ops, synthetic as syn

    cfg = configs.get("kitti")
    cam = cfg["camera"]
    B, N, K = batch, keypoints, frames
    gt = bt.kitti00_poses(K)
    gt = np.linalg.inv(gt[0]) @ gt
    schedule = bt.split_schedule(gt, cfg["split"]["local_map_distance"], cfg["split"]["local_map_angle_distance_radians"])
    longest = max(np.diff([0] + sorted(schedule) + [K])) + 6  # the estimate's splits may come a few frames off the ground truth's
    dev = torch.device("cuda", device)
    idx = torch.arange(B, device=dev) % unique
    if seqs is None:
        seqs = bt.make_sequences(cfg, unique, gt, N, syn.seed_for(1, 0) + 500000)
    stage = ops.StereoFrames(device, len(seqs), N, epilogue=False)
    inputs = []
    for k in range(K):
        for u, fr_list in enumerate(seqs):
            fr = fr_list[k]
            stage.upload(u, fr["uv_left"], fr["desc_left"], fr["uv_right"], fr["desc_right"])
        inputs.append(tuple(t.index_select(0, idx).contiguous() for t in (stage.left_kp, stage.left_desc, stage.right_kp, stage.right_desc, stage.n_left, stage.n_right)))
    del stage
    sf = ops.StereoFrames(device, B, N, epilogue=True)
    max_meas = int(longest) + 1
    maps = ops.MapBatch(device, B, cap, max_meas, max_meas + 1, N, N)
    maps.measurement, maps.measurement_desc, maps.n_measured = sf.fixed_uvuv, sf.fixed_desc, sf.n_fixed
    clip = ops.ClipScenes(device, B, cap)
    clip.scene_xyzw, clip.scene_desc, clip.n_scene, clip.scene_n_opt = maps.coords, maps.desc, maps.n_points, maps.n_opt
    af = ops.AlignFrames(device, B, N, cap)
    af.fixed, af.fixed_desc, af.n_fixed = sf.fixed_uvuv, sf.fixed_desc, sf.n_fixed
    af.moving, af.moving_desc, af.n_moving = clip.clipped_xyzw, clip.clipped_desc, clip.n_clipped
    af.max_fixed = max_fixed
    maps.corr, maps.corr_from_aligner, maps.scene_index_map = af.corr, 1, clip.global_indices
    nodes = len(schedule) + 8
    graphs = ops.PoseGraphBatch(device, B, nodes, nodes, envelope_blocks=2 * nodes)
    sess = ops.SessionBatch(device, maps, af, graphs, K)
    eye = torch.eye(4, dtype=torch.float32, device=dev).repeat(B, 1, 1).contiguous()
    ctx = ops.Context(device)
    sp, tp = ops.stereo_params(cfg["stereo_matcher"], cam["rows"]), ops.triangulator_params(cfg)
    pp, apar = ops.pcf_params(cfg), ops.aligner_params(cfg)
    if prior_info > 0:
        ops.set_motion_prior(apar, (prior_info,) * 6)
    mp = merger_params(cfg, ops.EST_SMOOTHER)
    params = ops.session_params(cfg["split"])
    I4 = np.eye(4, dtype=np.float32)
    worst = torch.zeros((3, B), dtype=torch.int32, device=dev)  # lowest status seen: session, merger, aligner
    n_splits = torch.zeros((B,), dtype=torch.int32, device=dev)
    warn_off = ops.AlignResult.warnings.offset

    def frame(k):
        sf.left_kp, sf.left_desc, sf.right_kp, sf.right_desc, sf.n_left, sf.n_right = inputs[k]
        ops.stereo_match_batch(ctx, sp, sf, tp)
        if k > 0:
            clip.robot_in_local_map.copy_(sess.prediction.view(B, 4, 4), non_blocking=True)
            af.X.copy_(eye.view(B, 16), non_blocking=True)
            ops.scene_clip_batch(ctx, pp.projector, I4, clip)
            ops.align_batch(ctx, pp, apar, af)
            torch.minimum(worst[2], af.result[:, warn_off: warn_off + 4].contiguous().view(torch.int32).view(B), out=worst[2])
        sess.step(ctx, params)
        ops.merge_batch(ctx, mp, maps)
        torch.minimum(worst[0], sess.status, out=worst[0])
        torch.minimum(worst[1], maps.result[:, 2], out=worst[1])
        n_splits.add_((sess.reason != 0).to(torch.int32))

    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ctx.use_torch_stream()
        frame(0)
        frame(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(2, K):
            frame(k)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        lows = worst.min(dim=1).values.cpu().numpy()
        if (lows < 0).any():
            raise SystemExit("a sequence reported an error: session %d, merger %d, aligner %d" % tuple(int(v) for v in lows))
        traj = sess.unroll(ctx).cpu().numpy().reshape(B, K, 4, 4)
        step_us, replaced_us = step_against_replaced(ctx, B, device=device)
    path_len = float(np.sum(np.linalg.norm(np.diff(gt[:, :3, 3], axis=0), axis=1)))
    drift = np.linalg.norm(traj[: min(unique, B), -1, :3, 3] - gt[-1][:3, 3], axis=1)
    splits = n_splits.cpu().numpy()
    out = {"batch": B, "frames": K, "frames_per_s": B * (K - 2) / elapsed, "ms_per_frame": elapsed / (K - 2) * 1e3,
           "session_step_us": step_us, "replaced_launches_us": replaced_us,
           "splits_per_sequence": [int(splits.min()), int(splits.max())], "splits_of_the_ground_truth_schedule": len(schedule),
           "end_point_drift_percent_of_path": [float(100.0 * d / path_len) for d in drift]}
    ctx.close()
    return out, seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,256,4096")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--unique", type=int, default=5)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--cap", type=int, default=6144)
    args = ap.parse_args()
    runs, seqs = [], None
    for b in (int(v) for v in args.batches.split(",")):
        r, seqs = run(b, args.frames, args.unique, args.keypoints, args.cap, seqs=seqs)
        runs.append(r)
    print(json.dumps({"metric": "closed tracking loop on KITTI-00 with per-sequence local-map management on the device", "runs": runs}))


if __name__ == "__main__":
    main()
