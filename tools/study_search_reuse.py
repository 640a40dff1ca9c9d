"""How often a later projective search could settle a query from what an earlier search of the same frame loop scanned (CPU only).

The search kernel's query cache (csrc/align.hip) serves a query when the cell rectangle it would scan now lies inside the rectangle
it scanned when its entry was written.  This tool measures that criterion -- and the stricter "projects to the same pixel" -- with
the CPU checker: the pose after k aligner iterations (max_iterations = k) stands in for the pose of a later search.

    python tools/study_search_reuse.py [config=kitti] [keypoints=2000] [frames=6]

Per pair (entry written at iteration a -> searched at iteration b): the smallest and largest share over the frames of visible
queries whose rectangle is contained / whose pixel is the same."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
from oracle import binding as ob  # noqa: E402
from srrg2_proslam_amd import configs, synthetic as syn  # noqa: E402

ITERATIONS = (0, 1, 5, 10, 15)
PAIRS = ((0, 1), (1, 5), (5, 10), (10, 15), (1, 10), (1, 15))
CELL = 4  # log2 of the cell edge in pixels


def poses_of(cfg, d, iterations):
    """the frame's pose after k aligner iterations, for every k"""
    sp, tp, pp, ap = bench.oracle_params(cfg)
    fr, mp = d["fr"], d["mp"]
    if sp is not None:
        corr, _ = ob.stereo_match(fr["uv_left"], fr["desc_left"], fr["uv_right"], fr["desc_right"], sp)
        fixed, src = ob.stereo_assemble(fr["uv_left"], fr["uv_right"], corr)
        ob.triangulate(fixed, tp)
        fdesc = fr["desc_left"][src]
        ap.mean_disparity = ob.mean_disparity(fixed)
    else:
        fixed, fdesc = fr["fixed"], fr["desc_fixed"]
    out = {}
    for k in iterations:
        if k == 0:
            out[k] = np.asarray(d["X0"], np.float32).reshape(4, 4)
            continue
        ap.max_iterations = k
        finder = ob.ProjectiveFinder(pp)
        finder.set_fixed(fixed, fdesc)
        finder.set_moving(mp["xyz"], mp["desc"])
        res, _ = ob.align_frame(finder, ap, fixed, mp["xyz"], ob.info_scale_from_nopt(mp["n_opt"]), d["X0"])
        finder.close()
        out[k] = np.array(res.X, np.float32).reshape(4, 4)
    return out


def rectangles(cfg, xyz, X, radius):
    """(cell rectangle cx0, cx1, cy0, cy1; pixel col, row; visible) of every query under pose X: the kernel's projection, rounding,
    clamps and cells in float32"""
    cam = cfg["camera"]
    p = np.asarray(xyz, np.float32)[:, :3]
    q = ((X[:3, 0] * p[:, :1] + X[:3, 1] * p[:, 1:2]) + X[:3, 2] * p[:, 2:3]) + X[:3, 3]
    z = q[:, 2]
    with np.errstate(all="ignore"):
        u = (np.float32(cam["fx"]) * q[:, 0] + np.float32(cam["cx"]) * z) / z
        v = (np.float32(cam["fy"]) * q[:, 1] + np.float32(cam["cy"]) * z) / z
    cols, rows = cam["cols"], cam["rows"]
    visible = (z >= np.float32(cfg["projector"]["range_min"])) & (z <= np.float32(cfg["projector"]["range_max"])) & (u >= 0) & (u < cols) & (v >= 0) & (v < rows)
    col, row = np.rint(np.where(visible, u, 0)).astype(np.int64), np.rint(np.where(visible, v, 0)).astype(np.int64)
    colmax = (((cols + (1 << CELL) - 1) >> CELL) << CELL) - 1
    rect = np.stack([np.maximum(col - radius, 0) >> CELL, np.minimum(col + radius, colmax) >> CELL,
                     np.maximum(row - radius, 0) >> CELL, np.minimum(row + radius, rows - 1) >> CELL], axis=1)
    return rect, np.stack([col, row], axis=1), visible


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "kitti"
    n_kp = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    n_frames = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    cfg = configs.get(name)
    ob.lib()
    radius = int(cfg["projective_finder"]["maximum_search_radius_pixels"])
    frames = bench.make_unique_frames(cfg, n_frames, n_kp, n_kp, syn.seed_for(1, 0))
    shares = {pair: [] for pair in PAIRS}
    for d in frames:
        poses = poses_of(cfg, d, ITERATIONS)
        geo = {k: rectangles(cfg, d["mp"]["xyz"], X, radius) for k, X in poses.items()}
        for a, b in PAIRS:
            (ra, pa, va), (rb, pb, vb) = geo[a], geo[b]
            contained = va & vb & (rb[:, 0] >= ra[:, 0]) & (rb[:, 1] <= ra[:, 1]) & (rb[:, 2] >= ra[:, 2]) & (rb[:, 3] <= ra[:, 3])
            same = va & vb & (pa == pb).all(axis=1)
            shares[(a, b)].append((contained.sum() / max(vb.sum(), 1), same.sum() / max(vb.sum(), 1)))
    print("%s, %d keypoints, %d frames, radius %d, %d-px cells" % (name, n_kp, n_frames, radius, 1 << CELL))
    print("| entry written at -> searched at | contained | same pixel |")
    print("|---|---|---|")
    for (a, b), v in shares.items():
        c, s = np.array(v)[:, 0], np.array(v)[:, 1]
        print("| it %d -> it %d | %.2f - %.2f | %.2f - %.2f |" % (a, b, c.min(), c.max(), s.min(), s.max()))


if __name__ == "__main__":
    main()
