"""closure merger throughput: B (scene, measurement) pairs resident in HBM, one launch per measurement
usage: python tools/bench_closure_merge.py [--batches 1,8,64,512,4096] [--iters 20] [--json out.json]
shapes: "icl"   321 landmarks, 338 (u, v, d) measurements, 282 correspondences (the frames of the reference's two merger gtests)
        "kitti" 145 landmarks, 139 XYZ measurements, the brute-force matcher's correspondences of city 01 against city 00
every launch merges into a fresh copy of the scenes (the copy is timed apart and subtracted); for orientation the same ICL frame
goes through prs_merge_batch_run (depth EKF, the tracking merger) in the same run.  The chain row is matcher -> loop aligner ->
closure merger on a LoopClosureBatch of the KITTI shape, back to back on one stream."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from srrg2_proslam_amd import _lib, configs, ops  # noqa: E402


def _time(fn, reset, iters):
    """mean ms of fn() over iters runs, each after reset(); the resets' own time is measured apart and subtracted"""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    reset()
    fn()
    torch.cuda.synchronize()
    e[0].record()
    for _ in range(iters):
        reset()
    e[1].record()
    for _ in range(iters):
        reset()
        fn()
    e[2].record()
    torch.cuda.synchronize()
    return (e[1].elapsed_time(e[2]) - e[0].elapsed_time(e[1])) / iters


def shapes():
    import closure_merge_cases as cc
    import closure_merge_ref as cr
    import point_align_ref as par
    from oracle import binding as ob
    from test_ref_pins import OracleBackend
    B = OracleBackend()
    icl = cc.icl_case(B, "01", 0.25, 200, 1)
    k = {s["name"]: s for s in par.scenarios(B)}["kitti_00_01"]
    corr, _ = ob.bruteforce_match(k["fixed_desc"], k["moving_desc"], 25.0, 0.9)
    kc = configs.get("kitti")
    P = ops.closure_merger_params(kc["closure_merger"], kc["camera"], "xyz")
    Pd = {f: getattr(P, f) for f, _ in _lib.ClosureMergerParams._fields_}
    kitti = dict(P=Pd, scene=cr.make_scene(512, k["moving"], k["moving_desc"]), measurement=cc.rows4(k["fixed"]), measurement_desc=k["fixed_desc"],
                 corr=corr.astype(cr.CORR_DTYPE), transform=np.linalg.inv(k["truth"]).astype(np.float32), scene_in_world=np.eye(4, dtype=np.float32),
                 transform_is_scene_in_measurement=1, corr_from_aligner=1)
    return {"icl": icl, "kitti": kitti}, k


def bench_shape(ctx, name, c, batches, iters):
    rows = []
    P = _lib.ClosureMergerParams()
    for f, v in c["P"].items():
        setattr(P, f, v)
    for B in batches:
        mb = ops.ClosureMergeBatch(0, B, c["scene"]["coords"].shape[0], len(c["measurement"]), len(c["corr"]))
        mb.corr_from_aligner, mb.transform_is_scene_in_measurement = c.get("corr_from_aligner", 0), c.get("transform_is_scene_in_measurement", 0)
        mb.upload(0, c["scene"], c["measurement"], c["measurement_desc"], c["corr"], c["transform"], c.get("scene_in_world"))
        names = ("coords", "desc", "n_points", "state", "covariance", "n_opt", "inlier", "n_meas", "scene_in_world", "measurement",
                 "measurement_desc", "n_measured", "corr", "n_corr", "transform")
        for n in names:
            t = getattr(mb, n)
            t[1:] = t[0]
        keep = {n: getattr(mb, n).clone() for n in names[:8]}

        def reset():
            for n, t in keep.items():
                getattr(mb, n).copy_(t)

        ms = _time(lambda: ops.closure_merge_batch(ctx, P, mb), reset, iters)
        res = mb.result.cpu().numpy()
        assert (res == res[0]).all() and res[0, 2] == 0, res[0]
        rows.append(dict(shape=name, pairs=B, ms_per_launch=ms, us_per_pair=1e3 * ms / B, merged=int(res[0, 0]), added=int(res[0, 1])))
        print("%-6s B=%5d  %8.3f ms/launch  %8.2f us/pair  (merged %d, added %d per pair)" % (name, B, ms, 1e3 * ms / B, res[0, 0], res[0, 1]))
        del mb, keep
        torch.cuda.empty_cache()
    return rows


def bench_depth_ekf(ctx, c, batches, iters):
    """the tracking merger (PRS_MERGER_DEPTH_EKF) on the same ICL frame: the existing kernel beside the new one"""
    from oracle import binding_mapping as om
    from test_oracle_mapping import merger_params
    import ref_pins as rp
    Ki = (rp.ICL_K["fx"], rp.ICL_K["fy"], rp.ICL_K["cx"], rp.ICL_K["cy"])
    est = om.estimator_params(om.EST_EKF, 3, Ki, max_dist2=0.01)
    op = merger_params(dict(configs.get("icl")), om.MERGER_DEPTH_EKF, est, row_bins=10, col_bins=30, max_appearance=50.0, target_merges=200)
    P = _lib.MergerParams.from_buffer_copy(bytes(op))  # (the checker's struct has the layout of prs_merger_params)
    rows = []
    n, nm, nc = c["scene"]["n_points"], len(c["measurement"]), len(c["corr"])
    for B in batches:
        mb = ops.MapBatch(0, B, 512, 0, 4, nm, nc)
        dev = mb.coords.device
        mb.coords[:, :n] = torch.from_numpy(c["scene"]["coords"][:n]).to(dev)
        mb.state[:, :n] = torch.from_numpy(c["scene"]["coords"][:n]).to(dev)
        mb.desc[:, :n] = torch.from_numpy(c["scene"]["desc"][:n]).to(dev)
        mb.n_points.fill_(n)
        mb.measurement[:] = torch.from_numpy(c["measurement"]).to(dev)
        mb.measurement_desc[:] = torch.from_numpy(np.ascontiguousarray(c["measurement_desc"])).to(dev)
        mb.n_measured.fill_(nm)
        mb.corr[:] = torch.from_numpy(np.ascontiguousarray(c["corr"]).view(np.int32).reshape(-1, 3).copy()).to(dev)
        mb.n_corr.fill_(nc)
        names = ("coords", "desc", "state", "covariance", "n_opt", "inlier", "n_meas", "n_points")
        keep = {k: getattr(mb, k).clone() for k in names}

        def reset():
            for k, t in keep.items():
                getattr(mb, k).copy_(t)

        ms = _time(lambda: ops.merge_batch(ctx, P, mb), reset, iters)
        res = mb.result.cpu().numpy()
        rows.append(dict(shape="icl depth EKF (prs_merge_batch_run)", pairs=B, ms_per_launch=ms, us_per_pair=1e3 * ms / B, merged=int(res[0, 0]),
                         added=int(res[0, 1]), status=int(res[0, 2])))
        print("icl depth EKF (tracking merger) B=%5d  %8.3f ms/launch  %8.2f us/pair  (merged %d, added %d, status %d)" % (
            B, ms, 1e3 * ms / B, res[0, 0], res[0, 1], res[0, 2]))
        del mb, keep
        torch.cuda.empty_cache()
    return rows


def bench_chain(ctx, k, batches, iters):
    kc = configs.get("kitti")
    P = ops.closure_merger_params(kc["closure_merger"], kc["camera"], "xyz")
    bp, ap = ops.bruteforce_params(kc["loop"]["maximum_descriptor_distance"], 0.9), ops.point_align_params(kc["loop"])
    rows = []
    for B in batches:
        lc = ops.LoopClosureBatch(0, B, len(k["fixed"]), 512)
        lc.upload(0, k["fixed"], k["fixed_desc"], k["moving"], k["moving_desc"])
        for t in (lc.clouds.fixed_desc, lc.clouds.moving_desc, lc.clouds.n_fixed, lc.clouds.n_moving, lc.pairs.fixed, lc.pairs.moving,
                  lc.pairs.n_fixed, lc.pairs.n_moving):
            t[1:] = t[0]
        mb = ops.ClosureMergeBatch.from_closures(lc)
        keep = [(t, t.clone()) for t in (lc.pairs.moving, lc.clouds.moving_desc, lc.pairs.n_moving, lc.pairs.X)]

        def reset():
            for t, saved in keep:
                t.copy_(saved)

        def chain():
            lc.run(ctx, bp, ap)
            ops.closure_merge_batch(ctx, P, mb)

        ms_all = _time(chain, reset, iters)
        ms_front = _time(lambda: lc.run(ctx, bp, ap), reset, iters)
        res = mb.result.cpu().numpy()
        rows.append(dict(shape="kitti chain", pairs=B, ms_per_launch=ms_all, ms_matcher_and_aligner=ms_front, us_per_pair=1e3 * ms_all / B,
                         merged=int(res[0, 0]), added=int(res[0, 1])))
        print("kitti chain B=%5d  %8.3f ms matcher + aligner + merger, %8.3f ms matcher + aligner alone  (merged %d, added %d per pair)" % (
            B, ms_all, ms_front, res[0, 0], res[0, 1]))
        del lc, mb, keep
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64,512,4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    import __graft_entry__ as g
    g.build()
    cases, k = shapes()
    ctx = ops.Context(0)
    rows = []
    for name in ("icl", "kitti"):
        rows += bench_shape(ctx, name, cases[name], batches, a.iters)
    rows += bench_depth_ekf(ctx, cases["icl"], batches, a.iters)
    rows += bench_chain(ctx, k, batches, a.iters)
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
