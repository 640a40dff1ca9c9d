"""Merger test cases shared by tests/test_mapping_ref.py (CPU, the checker against float64) and tests/test_merge_dispatch_gpu.py
(the kernels against the checker and against float64): a static cloud of world points seen from a camera that moves through a
LOCAL MAP whose origin L is far from the world's (a rotation of tens of degrees about a skew axis, tens of metres away), so that
    measurement_in_world = L * motion_k,   measurement_in_scene = L^-1 * measurement_in_world != measurement_in_world
and world_in_local_map = measurement_in_scene * measurement_in_world^-1 (landmark_estimator_base.hpp:54) is far from the identity.
Measurements are the projections of the cloud with pixel noise and a few gross outliers; correspondences pair a landmark with
the measurement of the same world point (the point's number is the first four bytes of its descriptor)."""
import numpy as np

from oracle import binding as ob
from oracle import binding_mapping as om
from srrg2_proslam_amd import configs
from tests import ref_filters
from tests.test_oracle_mapping import merger_params as oracle_merger_params

# kind -> (estimator, measurement dim, merger, camera, history slots per landmark)
KINDS = {
    "weighted_mean": (om.EST_WEIGHTED_MEAN, 4, om.MERGER_STEREO_TRIANGULATION, "kitti", 0),
    "smoother": (om.EST_SMOOTHER, 4, om.MERGER_STEREO_TRIANGULATION, "kitti", 8),
    "stereo_ekf": (om.EST_EKF, 4, om.MERGER_STEREO_EKF, "kitti", 0),
    "depth_ekf": (om.EST_EKF, 3, om.MERGER_DEPTH_EKF, "icl", 0),
    "mono_ekf": (om.EST_EKF, 2, om.MERGER_DEPTH_EKF, "filters", 0),  # updates only: no merger adds points from (u, v)
}


def camera(kind):
    name = KINDS[kind][3]
    if name == "filters":  # tests/ref_filters.py: fx = fy = 450, 640 x 480
        K = ref_filters.K
        return {"fx": K[0], "fy": K[1], "cx": K[2], "cy": K[3], "rows": ref_filters.ROWS, "cols": ref_filters.COLS, "baseline_m": 0.0}
    return configs.get(name)["camera"]


def merger_params(kind, binning=1, **kw):
    """the estimator settings of tests/test_mapping_gpu.py (kitti.conf / icl.conf) and, for the mono filter, of tests/ref_filters.py"""
    est, dim, variant, cam_name, _ = KINDS[kind]
    if kind == "mono_ekf":
        p = ref_filters.merger_params(2)  # (target_number_of_merges stays 0: the form adds no points)
        p.enable_binning = binning
        p.number_of_row_bins, p.number_of_col_bins = kw.get("row_bins", 10), kw.get("col_bins", 10)
        return p
    cfg = configs.get(cam_name)
    cam = cfg["camera"]
    K = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    e = {"weighted_mean": dict(max_dist2=25.0), "smoother": dict(max_dist2=100.0, chi2_delta=1e-6), "depth_ekf": dict(max_dist2=1.0),
         "stereo_ekf": dict(baseline_px=(configs.baseline_pixels(cfg), 0.0), max_dist2=25.0, max_cov_norm2=0.25)}[kind]
    e.update(kw.pop("estimator", {}))
    kw.setdefault("target_merges", 10 ** 6)
    return oracle_merger_params(cfg, variant, om.estimator_params(est, dim, K, **e), enable_binning=binning, **kw)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def local_map_origin(rng):
    """L: 20..60 degrees about an axis with no zero component, 20..80 m away along every axis"""
    L = np.eye(4)
    L[:3, :3] = rotation(rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3), np.deg2rad(rng.uniform(20.0, 60.0)))
    L[:3, 3] = rng.uniform(20.0, 80.0, 3) * rng.choice([-1.0, 1.0], 3)
    return L


class Sequence:
    """one map's frames.  scene_is_world: measurement_in_scene = measurement_in_world (the metamorphic twin of the same case);
    no_corr: never any correspondence; empty_frame: index of a frame without measurements; far: depths up to 150 m"""

    def __init__(self, kind, seed, n_world, n_frames, scene_is_world=False, no_corr=False, empty_frame=None, far=False, noise=0.3,
                 outliers=0.03, response_max=70):
        self.kind, self.n_frames, self.no_corr, self.response_max = kind, n_frames, no_corr, response_max
        self.scene_is_world = scene_is_world
        self.dim, self.max_meas = KINDS[kind][1], KINDS[kind][4]
        rng = np.random.default_rng(seed)
        cam = camera(kind)
        self.L = local_map_origin(rng)
        small = KINDS[kind][3] != "kitti"  # indoor scale
        zr = (1.0, 6.0) if small else ((20.0, 150.0) if far else (6.0, 60.0))
        depth = rng.uniform(*zr, n_world)
        u, v = rng.uniform(30, cam["cols"] - 30, n_world), rng.uniform(20, cam["rows"] - 20, n_world)
        local = np.stack([(u - cam["cx"]) / cam["fx"] * depth, (v - cam["cy"]) / cam["fy"] * depth, depth], axis=1)
        self.local = local
        self.world = local @ self.L[:3, :3].T + self.L[:3, 3]
        self.desc = rng.integers(0, 256, (n_world, 32), dtype=np.uint8)
        self.desc[:, :4] = np.arange(n_world, dtype=np.uint32).view(np.uint8).reshape(n_world, 4)
        step = 0.05 if small else 0.6
        self.frames = []
        for k in range(n_frames):
            M = np.eye(4)
            M[:3, :3] = rotation((0, 1, 0), 0.02 * k) @ rotation((1, 0, 0), -0.01 * k)
            M[:3, 3] = np.array([0.08 * k, -0.03 * k, 1.0 * k]) * step + rng.normal(0, 0.01 * step, 3)
            Tw = (self.L @ M).astype(np.float32)
            Ts = Tw.copy() if scene_is_world else (np.linalg.inv(self.L) @ Tw.astype(np.float64)).astype(np.float32)
            Mi = np.linalg.inv(M)
            pc = local @ Mi[:3, :3].T + Mi[:3, 3]
            uu = cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"]
            vv = cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]
            ok = (pc[:, 2] > 0.5) & (uu > 2) & (uu < cam["cols"] - 2) & (vv > 2) & (vv < cam["rows"] - 2) & (rng.random(n_world) > 0.15)
            ids = rng.permutation(np.nonzero(ok)[0])
            if empty_frame == k:
                ids = ids[:0]
            n = len(ids)
            z = np.zeros((n, self.dim))
            z[:, 0], z[:, 1] = uu[ids] + rng.normal(0, noise, n), vv[ids] + rng.normal(0, noise, n)
            if self.dim == 4:
                z[:, 2] = uu[ids] - cam["fx"] * cam["baseline_m"] / pc[ids, 2] + rng.normal(0, noise, n)
                z[:, 3] = z[:, 1]
            elif self.dim == 3:
                z[:, 2] = pc[ids, 2] * (1.0 + rng.normal(0, 0.002, n))
            bad = rng.random(n) < outliers  # gross outliers: the estimators' gates have something to refuse
            if self.dim == 4:
                z[bad, 2] -= rng.uniform(3.0, 30.0, int(bad.sum()))
            else:
                z[bad, 0] += rng.uniform(5.0, 30.0, int(bad.sum()))
            self.frames.append({"Tw": Tw, "Ts": Ts, "z": z.astype(np.float32), "desc": self.desc[ids].copy(), "ids": ids,
                                "seed": seed * 1000 + k})

    def new_map(self, capacity):
        """the map before frame 0.  The mono filter only updates: its map starts with every world point (noisy, identity covariance)"""
        m = om.Map(capacity, self.max_meas)
        if self.kind == "mono_ekf":
            rng = np.random.default_rng(len(self.world))
            Li = np.eye(4) if self.scene_is_world else np.linalg.inv(self.L)
            for i in range(min(len(self.world), capacity)):
                w = (self.world[i] + rng.normal(0, 0.05, 3)).astype(np.float32)
                loc = (Li[:3, :3] @ w.astype(np.float64) + Li[:3, 3]).astype(np.float32)
                m.add_landmark(loc, w, np.eye(3, dtype=np.float32), desc=self.desc[i])
        return m

    def inputs(self, k, m, corr_stride=None):
        """-> (measurement_in_world, measurement_in_scene, measurement, descriptors, correspondences) of frame k for map m:
        every landmark whose world point is measured in this frame, in a random order, responses 0..response_max"""
        f = self.frames[k]
        corr = np.zeros(0, ob.CORR_DTYPE)
        if not self.no_corr and m.n_points > 0 and len(f["ids"]) > 0:
            meas_of = np.full(len(self.world), -1, np.int64)
            meas_of[f["ids"]] = np.arange(len(f["ids"]))
            world_id = np.ascontiguousarray(m.desc[: m.n_points, :4]).view(np.uint32).ravel()
            i = np.where(world_id < len(self.world), meas_of[np.minimum(world_id, len(self.world) - 1)], -1)  # (a foreign landmark matches nothing)
            s = np.nonzero(i >= 0)[0]
            rng = np.random.default_rng(f["seed"])
            s = rng.permutation(s)
            if corr_stride is not None:
                s = s[:corr_stride]
            corr = np.zeros(len(s), ob.CORR_DTYPE)
            corr["fixed_idx"], corr["moving_idx"] = s, i[s]
            corr["response"] = rng.integers(0, self.response_max, len(s)).astype(np.float32)
        return f["Tw"], f["Ts"], f["z"], f["desc"], corr


def distinct_batch(kind, n_maps=6, n_frames=5, seed=100, **kw):
    """n_maps different maps for one launch: sizes, seeds, poses and origins differ; map 1 never has correspondences, map 2 has an empty frame"""
    sizes = [160, 260, 90, 330, 40, 210, 120, 300]
    seqs = []
    for b in range(n_maps):
        seqs.append(Sequence(kind, seed + 17 * b, sizes[b % len(sizes)] + 3 * (b // len(sizes)), n_frames, no_corr=(b == 1),
                             empty_frame=(2 if b == 2 else None), **kw))
    return seqs
