"""Harness formats of the reference's benchmark tooling: trajectory files and a reader for
the subset of the BOSS `.conf` grammar the hot-path parameters live in.  Host-side plumbing, plain Python.

Trajectories (apps/app_benchmark.cpp:195-262):
  * a run keeps, per local map (keyframe), the stamped poses of the frames tracked in it, LOCAL to that map;
    `unroll_trajectory` composes `keyframe_estimate * local_pose` and orders by timestamp (`std::map::insert`:
    the first pose seen for a timestamp wins) (:195-203);
  * KITTI: one line per pose, the 3x4 matrix row-major, every value `std::fixed << std::setprecision(9)`
    followed by ONE space (also the last one), then a newline (:205-222, :244-250);
  * TUM: `timestamp tx ty tz qx qy qz qw ` in the same number format (:224-241, :252-259).  `t2tqxyzw` is part
    of srrg2_core (not in the reference tree): BUILD-DEFINED as translation + the unit quaternion of the rotation
    block by the usual trace / largest-diagonal branches, (x, y, z, w) order as the name says.
Values are float32 in the reference (`Isometry3f`); they are widened to double for printing, exactly what
`ostream << float` does, so a file written here is byte-identical to one written by the reference for the same
poses.

`.conf` files (configurations/*.conf): a sequence of `"ClassName" { ... }` records; a record body is a JSON
object with `//` comments, `"#id"` numbers the record, `{"#pointer": id}` refers to another record (-1 = none).
"""
import json
import math

import numpy as np


# ---------------------------------------------------------------- trajectories
def unroll_trajectory(local_maps):
    """local_maps: iterable of (keyframe_estimate [4,4], [(timestamp, local_pose [4,4]), ...]) ->
    list of (timestamp, global_pose float32 [4,4]) ordered by timestamp (app_benchmark.cpp:195-203)."""
    unrolled = {}
    for keyframe, stamped in local_maps:
        K = np.asarray(keyframe, np.float32).reshape(4, 4)
        for stamp, local in stamped:
            stamp = float(stamp)
            if stamp not in unrolled:  # std::map::insert keeps the entry already there
                unrolled[stamp] = (K @ np.asarray(local, np.float32).reshape(4, 4)).astype(np.float32)
    return [(s, unrolled[s]) for s in sorted(unrolled)]


def _fixed9(x):
    return "%.9f" % float(x)


def rotation_to_quaternion_xyzw(R):
    """unit quaternion (x, y, z, w) of a rotation matrix, float32 arithmetic (trace / largest-diagonal branches)."""
    m = np.asarray(R, np.float32).reshape(3, 3)
    f = np.float32
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > f(0):
        t = np.sqrt(t + f(1))
        w = f(0.5) * t
        t = f(0.5) / t
        x, y, z = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + f(1))
        q = [f(0), f(0), f(0)]
        q[i] = f(0.5) * t
        t = f(0.5) / t
        w = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
        x, y, z = q
    return np.array([x, y, z, w], np.float32)


def kitti_line(pose):
    """app_benchmark.cpp:244-250: twelve values, each followed by a space."""
    T = np.asarray(pose, np.float32).reshape(4, 4)
    return "".join(_fixed9(T[r, c]) + " " for r in range(3) for c in range(4))


def tum_line(stamp, pose):
    """app_benchmark.cpp:252-259: timestamp (double), translation, quaternion xyzw, each followed by a space."""
    T = np.asarray(pose, np.float32).reshape(4, 4)
    v = list(T[:3, 3]) + list(rotation_to_quaternion_xyzw(T[:3, :3]))
    return _fixed9(stamp) + " " + "".join(_fixed9(x) + " " for x in v)


def write_trajectory_kitti(path, stamped_poses):
    """stamped_poses: [(timestamp, pose [4,4])], already unrolled; ordered by timestamp on the way out."""
    with open(path, "w") as f:  # an unwritable path raises, like the reference (:211-214)
        for _, pose in sorted(stamped_poses, key=lambda e: e[0]):
            f.write(kitti_line(pose) + "\n")


def write_trajectory_tum(path, stamped_poses):
    with open(path, "w") as f:
        for stamp, pose in sorted(stamped_poses, key=lambda e: e[0]):
            f.write(tum_line(stamp, pose) + "\n")


def read_trajectory_kitti(path):
    """-> float64 [n, 4, 4] (last row 0 0 0 1)"""
    out = []
    with open(path) as f:
        for line in f:
            v = line.split()
            if not v:
                continue
            if len(v) != 12:
                raise ValueError("read_trajectory_kitti|expected 12 values per line, got %d" % len(v))
            T = np.eye(4)
            T[:3, :4] = np.array(v, np.float64).reshape(3, 4)
            out.append(T)
    return np.array(out).reshape(-1, 4, 4)


def read_trajectory_tum(path):
    """-> (timestamps float64 [n], poses float64 [n, 4, 4])"""
    stamps, poses = [], []
    with open(path) as f:
        for line in f:
            v = line.split()
            if not v or v[0].startswith("#"):
                continue
            if len(v) != 8:
                raise ValueError("read_trajectory_tum|expected 8 values per line, got %d" % len(v))
            ts, tx, ty, tz, qx, qy, qz, qw = (float(x) for x in v)
            n = math.sqrt(qx * qx + qy * qy + qz * qz + qw * qw)
            qx, qy, qz, qw = qx / n, qy / n, qz / n, qw / n
            T = np.eye(4)
            T[:3, :3] = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                         [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                         [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]]
            T[:3, 3] = [tx, ty, tz]
            stamps.append(ts)
            poses.append(T)
    return np.array(stamps), np.array(poses).reshape(-1, 4, 4)


def associate(stamps_est, stamps_gt, max_difference=0.02):
    """TUM's association (associate.py) of an estimate's time stamps with a ground truth's: every pair closer than max_difference is a
    candidate, candidates are taken nearest first, and a stamp of either side is used once.  -> (gt_row int64 [n_est], the ground
    truth's row for each row of the estimate or -1, valid uint8 [n_est]).  gt[gt_row] with the mask is what the trajectory
    evaluator takes (ops.TrajectoryEvalBatch.set_ground_truth): the ICL / TUM / EuRoC route, whose ground truth has its own clock."""
    est = np.asarray(stamps_est, np.float64).reshape(-1)
    gt = np.asarray(stamps_gt, np.float64).reshape(-1)
    order = np.argsort(gt, kind="stable")
    sgt = gt[order]
    lo = np.searchsorted(sgt, est - max_difference, side="left")
    hi = np.searchsorted(sgt, est + max_difference, side="right")
    cand = [(abs(est[i] - sgt[j]), i, int(order[j])) for i in range(est.size) for j in range(lo[i], hi[i])
            if abs(est[i] - sgt[j]) < max_difference]
    cand.sort()
    gt_row = np.full(est.size, -1, np.int64)
    used = np.zeros(gt.size, bool)
    for _, i, j in cand:
        if gt_row[i] < 0 and not used[j]:
            gt_row[i] = j
            used[j] = True
    return gt_row, (gt_row >= 0).astype(np.uint8)


def write_ply(path, xyz, desc=None, normals=None, faces=None):
    """a minimal binary-little-endian PLY of a landmark cloud (ops.WorldMapBatch.cloud_of: xyz [n, 3] or [n, 4], the first three
    columns are written; desc: optional uint8 [n, 32], written as 32 uchar properties d0 .. d31 of every vertex; normals: optional
    [n, 3] or [n, 4] (ops.DepthNormalsBatch.rows_of), the first three columns written as nx ny nz behind x y z; faces: optional
    integer [m, 3] or [m, 4] of vertex rows (ops.TsdfMeshBatch.mesh_of), written behind the vertices as `element face m` with
    `property list uchar int vertex_indices`; an index outside [0, n) raises ValueError.  Without faces the file has no face
    element at all)"""
    xyz = np.asarray(xyz, np.float32)
    if xyz.ndim != 2 or xyz.shape[1] not in (3, 4):
        raise ValueError("xyz must be [n, 3] or [n, 4]")
    n = xyz.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if normals is not None else []) + \
        ([("d%d" % i, "u1") for i in range(32)] if desc is not None else [])
    rec = np.zeros(n, np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        normals = np.asarray(normals, np.float32)
        if normals.ndim != 2 or normals.shape[0] != n or normals.shape[1] not in (3, 4):
            raise ValueError("normals must be [n, 3] or [n, 4]")
        rec["nx"], rec["ny"], rec["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    if desc is not None:
        desc = np.asarray(desc, np.uint8)
        if desc.shape != (n, 32):
            raise ValueError("desc must be [n, 32]")
        for i in range(32):
            rec["d%d" % i] = desc[:, i]
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n]
    header += ["property %s %s" % ("float" if rec.dtype[name].kind == "f" else "uchar", name) for name in rec.dtype.names]
    face_rec = None
    if faces is not None:
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[1] not in (3, 4) or faces.dtype.kind not in "iu":
            raise ValueError("faces must be an integer [m, 3] or [m, 4]")
        if faces.size and (int(faces.min()) < 0 or int(faces.max()) >= n):
            raise ValueError("faces names a vertex outside [0, %d)" % n)
        face_rec = np.zeros(faces.shape[0], np.dtype([("count", "u1"), ("vertex_indices", "<i4", (faces.shape[1],))]))
        face_rec["count"], face_rec["vertex_indices"] = faces.shape[1], faces
        header += ["element face %d" % faces.shape[0], "property list uchar int vertex_indices"]
    with open(path, "wb") as f:
        f.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        f.write(rec.tobytes())
        if face_rec is not None:
            f.write(face_rec.tobytes())


# ---------------------------------------------------------------- .conf reader (subset)
def _strip_line_comments(text):
    out, in_string, i = [], False, 0
    while i < len(text):
        ch = text[i]
        if in_string:
            out.append(ch)
            if ch == "\\" and i + 1 < len(text):
                out.append(text[i + 1])
                i += 1
            elif ch == '"':
                in_string = False
        elif ch == '"':
            in_string = True
            out.append(ch)
        elif ch == "/" and text[i + 1:i + 2] == "/":
            while i < len(text) and text[i] != "\n":
                i += 1
            continue
        else:
            out.append(ch)
        i += 1
    return "".join(out)


class ConfRecord(dict):
    """one `"ClassName" { ... }` record: a dict of its fields plus `.class_name` and `.id`"""

    def __init__(self, class_name, fields):
        super().__init__(fields)
        self.class_name = class_name
        self.id = fields.get("#id")


class Conf:
    """records of a `.conf` file in file order, by id, by `name` field and by class"""

    def __init__(self, records):
        self.records = records
        self.by_id = {r.id: r for r in records if r.id is not None}
        self.by_name = {r["name"]: r for r in records if isinstance(r.get("name"), str) and r.get("name")}

    def of_class(self, class_name):
        return [r for r in self.records if r.class_name == class_name]

    def deref(self, value):
        """`{"#pointer": id}` -> the record (None for -1 / unknown ids); anything else is returned as it is"""
        if isinstance(value, dict) and "#pointer" in value:
            return self.by_id.get(value["#pointer"])
        return value

    def follow(self, record, *fields):
        """record.field1 -> pointer -> .field2 -> ... ; None as soon as a link is missing"""
        cur = record
        for name in fields:
            if cur is None or name not in cur:
                return None
            cur = self.deref(cur[name])
        return cur


def parse_conf(text):
    """-> Conf.  Raises ValueError on text that is not a sequence of `"ClassName" { json }` records."""
    clean = _strip_line_comments(text)
    dec = json.JSONDecoder()
    pos, records = 0, []
    while True:
        while pos < len(clean) and clean[pos].isspace():
            pos += 1
        if pos >= len(clean):
            break
        try:
            class_name, pos = dec.raw_decode(clean, pos)
            while pos < len(clean) and clean[pos].isspace():
                pos += 1
            fields, pos = dec.raw_decode(clean, pos)
        except json.JSONDecodeError as e:
            raise ValueError("parse_conf|not a record at offset %d: %s" % (pos, e)) from None
        if not isinstance(class_name, str) or not isinstance(fields, dict):
            raise ValueError("parse_conf|expected \"ClassName\" { ... } at offset %d" % pos)
        records.append(ConfRecord(class_name, fields))
    return Conf(records)


def read_conf(path):
    with open(path) as f:
        return parse_conf(f.read())


_SEARCH_CLASSES = (("CorrespondenceFinderProjectiveKDTree", 0), ("CorrespondenceFinderProjectiveSquare", 1),
                   ("CorrespondenceFinderProjectiveCircle", 2), ("CorrespondenceFinderProjectiveRhombus", 3))
_SLICE_FACTORS = (("AlignerSliceProcessorProjectiveStereo", 4), ("AlignerSliceProcessorProjectiveDepth", 3),
                  ("AlignerSliceProcessorProjective", 2))  # error dimension of the slice's factor (configs.FACTOR_*)


def _pick(record, keys):
    return {k: record[k] for k in keys if k in record}


def hot_path_params(conf):
    """the hot-path parameter groups of a parsed configuration, in the shape of `configs.py`'s dictionaries,
    following the file's own wiring: stereo adaptor -> epipolar finder; projective slice processor -> finder,
    projector, robustifier; the aligner is the MultiAligner whose `slice_processors` hold that slice.
    Only fields present in the file are returned (the reference fills the rest with its class defaults)."""
    out = {}
    adaptor = next((r for r in conf.records if r.class_name.startswith("RawDataPreprocessorStereoProjective")), None)
    matcher = conf.follow(adaptor, "correspondence_finder") if adaptor is not None else None
    if matcher is not None:
        out["stereo_matcher"] = _pick(matcher, ("maximum_descriptor_distance", "maximum_distance_ratio_to_second_best",
                                                "minimum_matching_ratio", "maximum_disparity_pixels", "epipolar_line_thickness_pixels"))
    tri = next((r for r in conf.records if r.class_name.startswith("TriangulatorRigidStereo")), None)
    if tri is not None:
        out["triangulator"] = _pick(tri, ("minimum_disparity_pixels", "infinity_depth_meters"))
    slice_record, factor = None, None
    for prefix, dim in _SLICE_FACTORS:
        slice_record = next((r for r in conf.records if r.class_name.startswith(prefix)), None)
        if slice_record is not None:
            factor = dim
            break
    if slice_record is None:
        return out
    finder = conf.follow(slice_record, "finder")
    if finder is not None:
        d = _pick(finder, ("maximum_descriptor_distance", "maximum_distance_ratio_to_second_best", "minimum_matching_ratio",
                           "minimum_descriptor_distance", "descriptor_distance_step_size_pixels", "maximum_search_radius_pixels",
                           "minimum_search_radius_pixels", "search_radius_step_size_pixels", "minimum_number_of_iterations",
                           "maximum_estimate_change_norm_for_convergence", "number_of_solver_iterations_per_projection"))
        for prefix, kind in _SEARCH_CLASSES:
            if finder.class_name.startswith(prefix):
                d["search_type"] = kind
        out["projective_finder"] = d
    projector = conf.follow(slice_record, "projector")
    if projector is not None:
        out["projector"] = _pick(projector, ("range_min", "range_max"))
    al = {"factor_type": factor}
    if "diagonal_info_matrix" in slice_record:
        al["diagonal_info"] = tuple(slice_record["diagonal_info_matrix"])
    al.update(_pick(slice_record, ("enable_inverse_depth_weighting", "min_num_correspondences")))
    robustifier = conf.follow(slice_record, "robustifier")
    if robustifier is not None and "chi_threshold" in robustifier:
        al["chi_threshold"] = robustifier["chi_threshold"]
    for r in conf.records:
        if r.class_name.startswith("MultiAligner") and any(conf.deref(p) is slice_record for p in r.get("slice_processors", [])):
            al.update(_pick(r, ("max_iterations", "min_num_inliers", "enable_inlier_only_runs", "keep_only_inlier_correspondences")))
            algorithm = conf.follow(r, "solver", "algorithm")
            if algorithm is not None and "damping" in algorithm:
                al["damping"] = algorithm["damping"]
            break
    out["aligner"] = al
    return out


_ROBUSTIFIERS = (("RobustifierSaturated", "saturated"), ("RobustifierClamp", "clamp"))
_VERDICT = ("relocalize_min_inliers", "relocalize_min_inliers_ratio", "relocalize_max_chi_inliers")


def loop_params(conf):
    """the loop aligner's parameter group of a parsed configuration, following the file's own wiring: MultiLoopDetectorHBST3D ->
    relocalize_aligner (a MultiAligner) -> its AlignerSliceProcessor3D -> robustifier class and chi_threshold; the aligner's solver
    -> algorithm damping; the detector's maximum_descriptor_distance and verdict thresholds, and MultiRelocalizer3D's thresholds
    under "relocalizer".  Only fields present in the file are returned."""
    out = {}
    detector = next((r for r in conf.records if r.class_name.startswith("MultiLoopDetector")), None)
    if detector is not None:
        out.update(_pick(detector, ("maximum_descriptor_distance",) + _VERDICT))
        aligner = conf.follow(detector, "relocalize_aligner")
        if aligner is not None:
            out.update(_pick(aligner, ("max_iterations", "min_num_inliers", "enable_inlier_only_runs", "keep_only_inlier_correspondences")))
            for ptr in aligner.get("slice_processors", []):
                sl = conf.deref(ptr)
                if sl is None or not sl.class_name.startswith("AlignerSliceProcessor3D"):
                    continue
                out.update(_pick(sl, ("min_num_correspondences",)))
                robustifier = conf.follow(sl, "robustifier")
                if robustifier is not None:
                    for prefix, kind in _ROBUSTIFIERS:
                        if robustifier.class_name.startswith(prefix):
                            out["robustifier"] = kind
                    if "chi_threshold" in robustifier:
                        out["chi_threshold"] = robustifier["chi_threshold"]
                break
            solver = conf.follow(aligner, "solver")
            if solver is not None and "max_iterations" in solver:
                out["solver_iterations"] = solver["max_iterations"]
            algorithm = conf.follow(aligner, "solver", "algorithm")
            if algorithm is not None and "damping" in algorithm:
                out["damping"] = algorithm["damping"]
    relocalizer = next((r for r in conf.records if r.class_name.startswith("MultiRelocalizer")), None)
    if relocalizer is not None:
        out["relocalizer"] = _pick(relocalizer, _VERDICT)
    return out


_PLACE = ("maximum_descriptor_distance", "minimum_age_difference_to_candidates", "relocalize_min_inliers", "maximum_leaf_size",
          "maximum_depth", "maximum_partitioning", "maximum_distance_for_merge")


def place_params(conf):
    """the loop detector's candidate-search group of a parsed configuration (MultiLoopDetectorHBST*: correspondence_finder_hbst.h).
    maximum_leaf_size, maximum_depth and maximum_partitioning shape the HBST tree, which this build replaces by an exhaustive search:
    read, unused.  Only fields present in the file are returned."""
    detector = next((r for r in conf.records if r.class_name.startswith("MultiLoopDetector")), None)
    return _pick(detector, _PLACE) if detector is not None else {}


def graph_params(conf):
    """the global solver's parameter group of a parsed configuration (the pose-graph optimiser, include/proslam_hip.h
    prs_pose_graph_*), following the file's own wiring: MultiGraphSLAM* -> global_solver (a Solver: max_iterations) -> algorithm
    (IterationAlgorithmGN: damping), termination_criteria (SimpleTerminationCriteria: epsilon) and linear_solver (its class name);
    closure_validator as the file has it (0 = none).  Only fields present in the file are returned."""
    slam = next((r for r in conf.records if r.class_name.startswith("MultiGraphSLAM")), None)
    solver = conf.follow(slam, "global_solver") if slam is not None else None
    if solver is None:
        return {}
    out = _pick(solver, ("max_iterations",))
    algorithm = conf.follow(solver, "algorithm")
    if algorithm is not None:
        out["algorithm"] = algorithm.class_name
        out.update(_pick(algorithm, ("damping",)))
    criteria = conf.follow(solver, "termination_criteria")
    if criteria is not None:
        out.update(_pick(criteria, ("epsilon",)))
    linear = conf.follow(solver, "linear_solver")
    if linear is not None:
        out["linear_solver"] = linear.class_name
    out["closure_validator"] = 0 if conf.follow(slam, "closure_validator") is None else 1
    return out


_GRAPH_LM = ("lm_iterations_max", "step_high", "step_low", "tau", "user_lambda_init", "variable_damping")


def graph_lm_params(conf):
    """the Levenberg-Marquardt block of the global solver (prs_pose_graph_lm_params), by the same wiring as graph_params:
    MultiGraphSLAM* -> global_solver -> algorithm, when that is an IterationAlgorithmLM; {} for a file that wires another algorithm.
    Only fields present in the file are returned."""
    slam = next((r for r in conf.records if r.class_name.startswith("MultiGraphSLAM")), None)
    algorithm = conf.follow(slam, "global_solver", "algorithm") if slam is not None else None
    if algorithm is None or not algorithm.class_name.startswith("IterationAlgorithmLM"):
        return {}
    return _pick(algorithm, _GRAPH_LM)


_CLOSURE_MERGER = ("enable_binning", "maximum_distance_geometry_squared", "maximum_response", "target_number_of_merges")


def closure_merger_params(conf):
    """the closure merger's parameter group of a parsed configuration (include/proslam_hip.h prs_closure_*), following the file's
    own wiring: the tracker slice (the first record that holds a `closure_merger` pointer) -> that merger, a
    MergerCorrespondencePointIntensityDescriptor3f in every shipped file; its class name under "class".  Only fields present in
    the file are returned."""
    for r in conf.records:
        merger = conf.follow(r, "closure_merger")
        if isinstance(merger, ConfRecord):
            out = _pick(merger, _CLOSURE_MERGER)
            out["class"] = merger.class_name
            return out
    return {}


_SPLIT = ("local_map_distance", "local_map_angle_distance_radians")


def split_params(conf):
    """the local-map splitting criterion's group of a parsed configuration (include/proslam_hip.h prs_session_params), following the
    file's own wiring: the record that holds a `splitting_criterion` pointer (MultiGraphSLAM3D) -> that criterion, a
    LocalMapSplittingCriterionViewpoint3D in every shipped file; its class name under "class".  Only fields present in the file
    are returned."""
    for r in conf.records:
        criterion = conf.follow(r, "splitting_criterion")
        if isinstance(criterion, ConfRecord):
            out = _pick(criterion, _SPLIT)
            out["class"] = criterion.class_name
            return out
    return {}


_RELOCALIZER = ("max_translation",) + _VERDICT


def relocalizer_params(conf):
    """the re-entry gates of a parsed configuration (include/proslam_hip.h prs_reentry_params): the MultiRelocalizer* record's
    max_translation and its three verdict thresholds.  Only fields present in the file are returned."""
    relocalizer = next((r for r in conf.records if r.class_name.startswith("MultiRelocalizer")), None)
    return _pick(relocalizer, _RELOCALIZER) if relocalizer is not None else {}
