"""Closed tracking loop with the local-map manager on the device (matcher -> clip -> aligner -> session step -> merge, ops.SessionBatch)
against the same chain on the CPU oracle with tests/session_ref.py's rule, one merge per frame in the reference's order
(apps/app_benchmark.cpp:100-183).  B = 2: sequence 0 follows KITTI-00 poses 0-30, sequence 1 poses 6-36.

The keypoint count is chosen on the CPU (oracle_chain below, run without a device) so that the oracle's own run has no lost frame, at
least two splits per sequence and different split frames in the two sequences: with N_KEYPOINTS = 400 it splits at frames 12 and
24 in sequence 0 and at frames 12 and 23 in sequence 1 (SPLITS), every split by viewpoint.  The first splits coincide (the car's
speed hardly changes over these 37 poses); the second ones differ."""
import os
import sys

import numpy as np
import pytest

import session_cases as sc
import session_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_KEYPOINTS, N_FRAMES, FIRST = 400, 31, (0, 6)
CAP, MAX_MEAS, PRIOR = 2048, 20, 1.0
SPLITS = ([12, 24], [12, 23])
F = np.float32


def sequences():
    """the two sequences' stereo frames (tools/bench_tracking.py's corridor world along the ground-truth poses)"""
    import bench_tracking as bt
    from srrg2_proslam_amd import configs, synthetic as syn
    cfg = configs.get("kitti")
    gt = sc.kitti00(FIRST[1] + N_FRAMES)
    out = []
    for u, first in enumerate(FIRST):
        poses = np.linalg.inv(gt[first]) @ gt[first: first + N_FRAMES]
        out.append(bt.make_sequences(cfg, 1, poses, N_KEYPOINTS, syn.seed_for(7, u))[0])
    return cfg, out


def oracle_chain(cfg, frames):
    """one sequence on the CPU oracle -> per frame dict(pose, n_points, warnings, reason, status), and the final World"""
    from oracle import binding as ob
    from oracle import binding_mapping as om
    from helpers import aligner_params as oap, oracle_stereo_params, oracle_tri_params, pcf_params_from_cfg
    cam = cfg["camera"]
    K = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    p = om.MergerParams()
    p.variant, p.enable_binning = om.MERGER_STEREO_TRIANGULATION, 1
    p.number_of_row_bins, p.number_of_col_bins = 20, 60
    p.canvas_rows, p.canvas_cols = cam["rows"], cam["cols"]
    p.maximum_distance_appearance, p.target_number_of_merges, p.target_merge_ratio = 100.0, 10 ** 6, 0.5
    p.triangulator = oracle_tri_params(ob, cfg)
    p.fx, p.fy, p.cx, p.cy = K
    p.estimator = om.estimator_params(om.EST_SMOOTHER, 4, K, max_dist2=100.0, chi2_delta=1e-6)
    m, table = om.Map(CAP, MAX_MEAS), om.pose_table(MAX_MEAS + 1)
    I4 = np.eye(4, dtype=F)
    d, a = cfg["split"]["local_map_distance"], cfg["split"]["local_map_angle_distance_radians"]
    w = ref.World(1, len(frames), CAP, 8, 8)
    finder = ob.ProjectiveFinder(pcf_params_from_cfg(ob, cfg))
    log = []
    for k, fr in enumerate(frames):
        corr, _ = ob.stereo_match(fr["uv_left"], fr["desc_left"], fr["uv_right"], fr["desc_right"], oracle_stereo_params(ob, cfg["stereo_matcher"]))
        fixed, src = ob.stereo_assemble(fr["uv_left"], fr["uv_right"], corr)
        fdesc = fr["desc_left"][src]
        X, status, warnings, rc, gi = I4.copy(), 0, 0, np.zeros(0, ob.CORR_DTYPE), None
        if k > 0:
            xyzw = m.coords[: m.n_points].copy()
            xyzw[:, 3] = ob.info_scale_from_nopt(m.n_opt[: m.n_points])
            cx, cd, gi, _ = ob.scene_clip(pcf_params_from_cfg(ob, cfg).projector, w.prediction[0], I4, xyzw, m.desc[: m.n_points])
            finder.set_fixed(fixed, fdesc)
            finder.set_moving(cx[:, :3], cd)
            ap = oap(ob, cfg, mean_disparity=ob.mean_disparity(fixed))
            ap.enable_motion_prior = 1
            for i in range(6):
                ap.motion_prior_info[i] = PRIOR
            res, rc = ob.align_frame(finder, ap, fixed, cx[:, :3], cx[:, 3], I4)
            X, status, warnings = np.array(res.X, F).reshape(4, 4), res.status, res.warnings
        w.n_points[0] = m.n_points
        ref.step(w, d, a, X[None], [status], [warnings], [len(rc)])
        if w.reason[0] != ref.NO_SPLIT:  # the finished map leaves, the frame seeds the new one
            m, table = om.Map(CAP, MAX_MEAS), om.pose_table(MAX_MEAS + 1)
        c, imap = np.zeros(0, ob.CORR_DTYPE), None
        if w.n_corr_merge[0] > 0:
            c = rc.copy()
            c["fixed_idx"], c["moving_idx"] = rc["moving_idx"], rc["fixed_idx"]
            imap = np.concatenate([gi, np.zeros(CAP - len(gi), np.int32)])
        rcode, _ = om.merge(p, w.measurement_in_world[0], w.measurement_in_scene[0], table, int(w.frame[0]), m, fixed, fdesc, c, imap)
        assert rcode == 0, (k, rcode)
        log.append(dict(pose=w.pose[0].copy(), n_points=m.n_points, warnings=int(warnings), reason=int(w.reason[0]), status=int(w.status[0]),
                        lost=bool(k > 0 and (status != 1 or warnings < 0))))
    finder.close()
    return log, w


@pytest.fixture(scope="module")
def oracle_runs():
    cfg, seqs = sequences()
    return cfg, seqs, [oracle_chain(cfg, s) for s in seqs]


def test_oracle_run_meets_the_conditions_the_keypoint_count_was_chosen_for(oracle_runs):
    _, _, runs = oracle_runs
    splits = [[k for k, e in enumerate(log) if e["reason"] != ref.NO_SPLIT] for log, _ in runs]
    print("splits", splits)
    for log, _ in runs:
        assert not any(e["lost"] for e in log) and not any(e["status"] for e in log)
        assert all(e["reason"] in (ref.NO_SPLIT, ref.SPLIT_VIEWPOINT) for e in log)
    assert len(splits[0]) >= 2 and len(splits[1]) >= 2 and splits[0] != splits[1]
    assert (splits[0], splits[1]) == SPLITS


@pytest.mark.gpu
def test_closed_loop_matches_the_oracle_chain(oracle_runs, hip_ctx):
    import torch
    from bench_merge import merger_params
    from srrg2_proslam_amd import ops
    cfg, seqs, runs = oracle_runs
    cam, B, N = cfg["camera"], 2, N_KEYPOINTS
    hip_ctx.use_torch_stream()
    sf = ops.StereoFrames(0, B, N, epilogue=True)
    maps = ops.MapBatch(0, B, CAP, MAX_MEAS, MAX_MEAS + 1, N, N)
    maps.measurement, maps.measurement_desc, maps.n_measured = sf.fixed_uvuv, sf.fixed_desc, sf.n_fixed
    clip = ops.ClipScenes(0, B, CAP)
    clip.scene_xyzw, clip.scene_desc, clip.n_scene, clip.scene_n_opt = maps.coords, maps.desc, maps.n_points, maps.n_opt
    af = ops.AlignFrames(0, B, N, CAP)
    af.fixed, af.fixed_desc, af.n_fixed = sf.fixed_uvuv, sf.fixed_desc, sf.n_fixed
    af.moving, af.moving_desc, af.n_moving = clip.clipped_xyzw, clip.clipped_desc, clip.n_clipped
    maps.corr, maps.corr_from_aligner, maps.scene_index_map = af.corr, 1, clip.global_indices
    graphs = ops.PoseGraphBatch(0, B, 8, 8, envelope_blocks=36)
    sess = ops.SessionBatch(0, maps, af, graphs, N_FRAMES)
    sp, tp = ops.stereo_params(cfg["stereo_matcher"], cam["rows"]), ops.triangulator_params(cfg)
    pp, apar = ops.pcf_params(cfg), ops.aligner_params(cfg)
    ops.set_motion_prior(apar, (PRIOR,) * 6)
    mp, params = merger_params(cfg, ops.EST_SMOOTHER), ops.session_params(cfg["split"])
    I4 = np.eye(4, dtype=F)
    eye = torch.eye(4, dtype=torch.float32, device=af.X.device).reshape(1, 16).repeat(B, 1)
    for k in range(N_FRAMES):
        for b in range(B):
            fr = seqs[b][k]
            sf.upload(b, fr["uv_left"], fr["desc_left"], fr["uv_right"], fr["desc_right"])
        ops.stereo_match_batch(hip_ctx, sp, sf, tp)
        if k > 0:
            clip.robot_in_local_map.copy_(sess.prediction.view(B, 4, 4))
            af.X.copy_(eye)
            ops.scene_clip_batch(hip_ctx, pp.projector, I4, clip)
            ops.align_batch(hip_ctx, pp, apar, af)
        sess.step(hip_ctx, params)
        ops.merge_batch(hip_ctx, mp, maps)
        for b in range(B):
            want, got = runs[b][0][k], sess.result_of(b)
            assert got["pose"].tobytes() == want["pose"].tobytes(), (k, b, "pose")
            assert (got["reason"], got["status"]) == (want["reason"], want["status"]), (k, b)
            assert int(maps.n_points[b].item()) == want["n_points"] and int(maps.result[b, 2].item()) >= 0, (k, b, "map size")
            if k > 0:
                assert af.result_of(b).warnings == want["warnings"], (k, b, "flags")
    trajectory = sess.unroll(hip_ctx).cpu().numpy().reshape(B, N_FRAMES, 4, 4)
    for b in range(B):
        w = runs[b][1]
        n, e = int(w.n_nodes[0]), int(w.n_edges[0])
        assert (int(graphs.n_nodes[b].item()), int(graphs.n_edges[b].item())) == (n, e) and n >= 3
        assert graphs.X[b, :n].cpu().numpy().tobytes() == w.X[0, :n].tobytes()
        src, dst, Z, omega = graphs.edges_of(b)
        assert np.array_equal(src, w.src[0, :e]) and np.array_equal(dst, w.dst[0, :e])
        assert Z.tobytes() == w.Z[0, :e].tobytes() and omega.tobytes() == w.omega[0, :e].tobytes()
        assert sess.frame_node[b].cpu().numpy().tobytes() == w.frame_node[0].tobytes()
        assert sess.frame_pose[b].cpu().numpy().tobytes() == w.frame_pose[0].tobytes()
        assert trajectory[b].tobytes() == ref.unroll(w)[0].tobytes()
