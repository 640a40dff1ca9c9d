"""Hot-path parameter sets of the reference's shipped configurations.

Every value cites the .conf line it was read from (paths relative to /root/reference/configurations/).
These are plain data; nothing here reads the reference at run time.
"""
import copy
import math

SEARCH_KDTREE, SEARCH_SQUARE, SEARCH_CIRCLE, SEARCH_RHOMBUS = 0, 1, 2, 3
FACTOR_MONO, FACTOR_DEPTH, FACTOR_STEREO = 2, 3, 4

_SQRT_FLT_MAX = 1.84467e19  # kitti.conf:40 "infinity_depth_meters"


def _loop(robustifier, chi_threshold, max_iterations, min_num_correspondences, max_distance, detector, relocalizer):
    """the loop aligner's group: MultiAligner3DQR min_num_inliers 10 and IterationAlgorithmGN damping 0 in every shipped file.
    SUBSTITUTION: HBST (srrg_hbst, not in the tree) finds the correspondences in the reference; the brute-force matcher stands in
    with the detector's maximum_descriptor_distance and the matcher's class-default Lowe ratio 0.9
    (CF/correspondence_finder_descriptor_based_bruteforce.h:27-31)."""
    return {"robustifier": robustifier, "chi_threshold": chi_threshold, "damping": 0.0, "max_iterations": max_iterations,
            "min_num_inliers": 10, "min_num_correspondences": min_num_correspondences, "maximum_descriptor_distance": max_distance,
            "maximum_distance_ratio_to_second_best": 0.9, "relocalize_min_inliers": detector[0],
            "relocalize_min_inliers_ratio": detector[1], "relocalize_max_chi_inliers": detector[2],
            "relocalizer": {"relocalize_min_inliers": relocalizer[0], "relocalize_min_inliers_ratio": relocalizer[1],
                            "relocalize_max_chi_inliers": relocalizer[2]}}



def _place(max_distance, minimum_age, min_inliers):
    """the loop detector's candidate search (include/proslam_hip.h prs_place_*): MultiLoopDetectorHBST3D's
    maximum_descriptor_distance, minimum_age_difference_to_candidates and relocalize_min_inliers.  SUBSTITUTION: the HBST tree
    (srrg_hbst, not in the tree) is searched exhaustively; its leaf size 100, depth 16 and partitioning 0.1 (every shipped file) are
    read but unused, and maximum_distance_for_merge is 0 everywhere (nothing merged)."""
    return {"maximum_descriptor_distance": max_distance, "minimum_age_difference_to_candidates": minimum_age,
            "relocalize_min_inliers": min_inliers, "maximum_leaf_size": 100, "maximum_depth": 16, "maximum_partitioning": 0.1,
            "maximum_distance_for_merge": 0}


def _graph(algorithm, damping, lm=None):
    """the global solver of the pose graph (include/proslam_hip.h prs_pose_graph_*): MultiGraphSLAM3D.global_solver, a Solver with
    max_iterations [10] and SimpleTerminationCriteria epsilon 0.001 in every shipped file; closure_validator is null in all of them.
    kitti, euroc and malaga wire IterationAlgorithmGN with damping 1e-06 and SparseBlockLinearSolverCholeskyCholmod; icl and tum wire
    IterationAlgorithmLM, whose six values are the `lm` sub-dict (prs_pose_graph_lm_params; ops.pose_graph_algorithm picks the entry
    from `algorithm`), and SparseBlockLinearSolverCholeskyCSparse.  `damping` of the LM files is the Gauss-Newton files' 1e-06, not
    a value of theirs: it serves a caller who runs the Gauss-Newton entry on them anyway.  SUBSTITUTION: a direct float64 LDL^T on
    the row envelope stands in for both sparse linear solvers."""
    out = {"algorithm": algorithm, "damping": damping, "max_iterations": 10, "epsilon": 0.001}
    if lm is not None:
        out["lm"] = lm
    return out


def _closure_merger():
    """the tracker slice's closure_merger (include/proslam_hip.h prs_closure_*): a MergerCorrespondencePointIntensityDescriptor3f
    with the same four values in every shipped file; the bin counts are the class defaults of merger_projective.h:47-56 (the
    merger's own defaults live in srrg2_slam_interfaces, not in the tree), the canvas and camera matrix come from "camera"."""
    return {"enable_binning": 1, "maximum_distance_geometry_squared": 0.25, "maximum_response": 50, "target_number_of_merges": 200,
            "number_of_row_bins": 10, "number_of_col_bins": 30}


# icl.conf:665-685 and tum.conf:174-194 (IterationAlgorithmLM), the same values: lm_iterations_max :669 / :178, step_high :672 / :181,
# step_low :675 / :184, tau :678 / :187, user_lambda_init :681 / :190, variable_damping :684 / :193
def _lm():
    return {"lm_iterations_max": 100, "step_high": 0.666667, "step_low": 0.333333, "tau": 1e-05, "user_lambda_init": 0,
            "variable_damping": 1}


# LocalMapSplittingCriterionViewpoint3D, the `splitting_criterion` of MultiGraphSLAM3D (the local-map manager, include/proslam_hip.h
# prs_session_params): a new local map once the sensor is further than the distance, or turned by more than the angle, from the
# map's origin
def _split(distance, angle):
    return {"local_map_distance": distance, "local_map_angle_distance_radians": angle}


KITTI = {
    "name": "kitti",
    # tests/fixtures.hpp:810-816,1093-1094
    "camera": {"fx": 718.856, "fy": 718.856, "cx": 607.193, "cy": 185.216, "cols": 1241, "rows": 376,
               "baseline_m": 0.537166},
    "projector": {"range_min": 0.1, "range_max": 1000.0},  # kitti.conf:175-178
    # kitti.conf:484-501
    "stereo_matcher": {"maximum_descriptor_distance": 100.0, "maximum_distance_ratio_to_second_best": 0.5,
                       "minimum_matching_ratio": 0.3, "maximum_disparity_pixels": 100,
                       "epipolar_line_thickness_pixels": 0},
    # kitti.conf:29-49
    "triangulator": {"minimum_disparity_pixels": 1.0, "infinity_depth_meters": _SQRT_FLT_MAX},
    # kitti.conf:834-875
    "projective_finder": {"search_type": SEARCH_CIRCLE, "maximum_descriptor_distance": 75.0,
                          "maximum_distance_ratio_to_second_best": 0.8, "minimum_matching_ratio": 0.1,
                          "minimum_descriptor_distance": 25.0, "descriptor_distance_step_size_pixels": 5.0,
                          "maximum_search_radius_pixels": 50, "minimum_search_radius_pixels": 10,
                          "search_radius_step_size_pixels": 10, "minimum_number_of_iterations": 5,
                          "maximum_estimate_change_norm_for_convergence": 0.01,
                          "number_of_solver_iterations_per_projection": 5},
    # kitti.conf:262-308 (slice), :137-142 (robustifier), :310-315 (damping), :980-1010 (aligner)
    "aligner": {"factor_type": FACTOR_STEREO, "diagonal_info": (1.0, 2.0, 1.0), "chi_threshold": 25.0,
                "enable_inverse_depth_weighting": 1, "damping": 1.0, "max_iterations": 100,
                "min_num_inliers": 6, "min_num_correspondences": 10},
    # loop aligner (include/proslam_hip.h prs_point_align_*): kitti.conf:938-978 (MultiLoopDetectorHBST3D -> relocalize_aligner
    # MultiAligner3DQR "loop_aligner"), :380-408 (AlignerSliceProcessor3D + RobustifierClamp), :877-882 (IterationAlgorithmGN),
    # :91-110 (MultiRelocalizer3D)
    "loop": _loop("clamp", 3.0, 100, 30, 25.0, (25, 0.5, 2.0), (25, 0.5, 5.0)),
    "place": _place(25.0, 10, 25),  # kitti.conf:938-978
    # kitti.conf:895-936 (global_solver) -> Solver :420-444, IterationAlgorithmGN :826-832, SimpleTerminationCriteria :884-889
    "graph": _graph("IterationAlgorithmGN", 1e-06),
    "closure_merger": _closure_merger(),  # kitti.conf:335-337 (slice) -> :446-460
    "split": _split(10, 0.25),  # kitti.conf:925 (splitting_criterion) -> :542-550: distance :549, angle :546
    "depth": {"min": 4.0, "max": 80.0},
}

EUROC = {
    "name": "euroc",
    # apps/example_triangulate_rigid_stereo.cpp:132-133,148-149
    "camera": {"fx": 435.262, "fy": 435.262, "cx": 367.415, "cy": 252.171, "cols": 752, "rows": 480,
               "baseline_m": 0.110078},
    "projector": {"range_min": 0.1, "range_max": 1000.0},  # euroc.conf:218-221
    # euroc.conf:539-551
    "stereo_matcher": {"maximum_descriptor_distance": 75.0, "maximum_distance_ratio_to_second_best": 0.5,
                       "minimum_matching_ratio": 0.3, "maximum_disparity_pixels": 200,
                       "epipolar_line_thickness_pixels": 0},
    "triangulator": {"minimum_disparity_pixels": 1.0, "infinity_depth_meters": _SQRT_FLT_MAX},  # euroc.conf:185
    # euroc.conf:919-957
    "projective_finder": {"search_type": SEARCH_CIRCLE, "maximum_descriptor_distance": 100.0,
                          "maximum_distance_ratio_to_second_best": 0.8, "minimum_matching_ratio": 0.1,
                          "minimum_descriptor_distance": 25.0, "descriptor_distance_step_size_pixels": 5.0,
                          "maximum_search_radius_pixels": 100, "minimum_search_radius_pixels": 25,
                          "search_radius_step_size_pixels": 5, "minimum_number_of_iterations": 5,
                          "maximum_estimate_change_norm_for_convergence": 0.001,
                          "number_of_solver_iterations_per_projection": 5},
    # euroc.conf:463-470 (slice), :231-235 (robustifier), :694-698 (damping), :1-15 (aligner)
    "aligner": {"factor_type": FACTOR_STEREO, "diagonal_info": (1.0, 2.0, 1.0), "chi_threshold": 100.0,
                "enable_inverse_depth_weighting": 1, "damping": 1.0, "max_iterations": 100,
                "min_num_inliers": 6, "min_num_correspondences": 0},  # euroc.conf:493
    # euroc.conf: MultiLoopDetectorHBST3D.relocalize_aligner -> AlignerSliceProcessor3D + RobustifierSaturated, MultiRelocalizer3D
    "loop": _loop("saturated", 1.0, 100, 0, 50.0, (100, 0.9, 0.25), (100, 0.9, 100.0)),
    "place": _place(50.0, 5, 100),  # euroc.conf: MultiLoopDetectorHBST3D
    "graph": _graph("IterationAlgorithmGN", 1e-06),  # euroc.conf:641-651 (MultiGraphSLAM3D -> global_solver)
    "closure_merger": _closure_merger(),  # euroc.conf:898-900 (slice) -> :519
    "split": _split(1, 0.5),  # euroc.conf:631-639: distance :638, angle :635
    "depth": {"min": 1.0, "max": 15.0},
}

ICL = {
    "name": "icl",
    # tests/fixtures.hpp:577,763-764
    "camera": {"fx": 481.2, "fy": -481.0, "cx": 319.5, "cy": 239.5, "cols": 640, "rows": 480, "baseline_m": 0.0},
    "projector": {"range_min": 0.001, "range_max": 100.0},  # icl.conf:313-316
    "stereo_matcher": None,
    "triangulator": None,
    # icl.conf:321-359
    "projective_finder": {"search_type": SEARCH_CIRCLE, "maximum_descriptor_distance": 35.0,
                          "maximum_distance_ratio_to_second_best": 0.9, "minimum_matching_ratio": 0.2,
                          "minimum_descriptor_distance": 30.0, "descriptor_distance_step_size_pixels": 5.0,
                          "maximum_search_radius_pixels": 100, "minimum_search_radius_pixels": 25,
                          "search_radius_step_size_pixels": 5, "minimum_number_of_iterations": 5,
                          "maximum_estimate_change_norm_for_convergence": 0.01,
                          "number_of_solver_iterations_per_projection": 5},
    # icl.conf:566-570 (slice), :459-463 (robustifier), :295-299 (damping), :50-64 (aligner)
    "aligner": {"factor_type": FACTOR_DEPTH, "diagonal_info": (1.0, 1.0, 10.0), "chi_threshold": 10.0,
                "enable_inverse_depth_weighting": 0, "damping": 0.1, "max_iterations": 100,
                "min_num_inliers": 6, "min_num_correspondences": 0,  # icl.conf:584
                "enable_inlier_only_runs": 1, "keep_only_inlier_correspondences": 1},  # icl.conf:50-53, :57-59
    # icl.conf:1-29 (loop_aligner), :600-628 (slice + RobustifierClamp), :153-158 (damping), :197-237 (detector), :687-705 (relocalizer)
    "loop": _loop("clamp", 1.0, 10, 0, 35.0, (50, 0.5, 0.1), (100, 0.5, 1000.0)),
    "place": _place(35.0, 1, 50),  # icl.conf:197-240
    "graph": _graph("IterationAlgorithmLM", 1e-06, _lm()),  # icl.conf:797-807 (MultiGraphSLAM3D -> global_solver), LM :665-685
    "closure_merger": _closure_merger(),  # icl.conf:178-180 (slice) -> :773
    "split": _split(5, 3),  # icl.conf:546-554: distance :553, angle :550
    "depth": {"min": 0.5, "max": 6.0},
    # RawDataPreprocessorMonocularDepth (icl.conf:642-650) and its IntensityFeatureExtractorBinned3D (icl.conf:745-770)
    "rgbd": {"depth_scaling_factor_to_meters": 0.001, "detector_threshold": 5, "enable_non_maximum_suppression": 1,
             "number_of_detectors_vertical": 3, "number_of_detectors_horizontal": 3, "target_number_of_keypoints": 500},
}

TUM = {
    "name": "tum",
    # intrinsics are not in the reference: the customary fr1 values are used
    "camera": {"fx": 525.0, "fy": 525.0, "cx": 319.5, "cy": 239.5, "cols": 640, "rows": 480, "baseline_m": 0.0},
    "projector": {"range_min": 0.01, "range_max": 7.5},  # tum.conf:133-136
    "stereo_matcher": None,
    "triangulator": None,
    # tum.conf:498-536
    "projective_finder": {"search_type": SEARCH_CIRCLE, "maximum_descriptor_distance": 75.0,
                          "maximum_distance_ratio_to_second_best": 0.7, "minimum_matching_ratio": 0.1,
                          "minimum_descriptor_distance": 35.0, "descriptor_distance_step_size_pixels": 5.0,
                          "maximum_search_radius_pixels": 100, "minimum_search_radius_pixels": 25,
                          "search_radius_step_size_pixels": 5, "minimum_number_of_iterations": 5,
                          "maximum_estimate_change_norm_for_convergence": 1e-5,
                          "number_of_solver_iterations_per_projection": 5},
    # tum.conf:242-246 (slice), :167-171 (robustifier), :146-150 (damping), :90-104 (aligner)
    "aligner": {"factor_type": FACTOR_DEPTH, "diagonal_info": (1.0, 1.0, 10.0), "chi_threshold": 25.0,
                "enable_inverse_depth_weighting": 0, "damping": 0.1, "max_iterations": 100,
                "min_num_inliers": 6, "min_num_correspondences": 0,  # tum.conf:260
                "enable_inlier_only_runs": 1, "keep_only_inlier_correspondences": 1},  # tum.conf:90-93, :97-99
    # tum.conf: MultiLoopDetectorHBST3D.relocalize_aligner -> AlignerSliceProcessor3D + RobustifierClamp, MultiRelocalizer3D
    "loop": _loop("clamp", 0.25, 10, 0, 25.0, (40, 0.5, 0.05), (40, 0.5, 100.0)),
    "place": _place(25.0, 1, 40),  # tum.conf: MultiLoopDetectorHBST3D
    "graph": _graph("IterationAlgorithmLM", 1e-06, _lm()),  # tum.conf:453-463 (MultiGraphSLAM3D -> global_solver), LM :174-194
    "closure_merger": _closure_merger(),  # tum.conf:221-223 (slice) -> :437
    "split": _split(1, 0.25),  # tum.conf:539-547: distance :546, angle :543
    "depth": {"min": 0.5, "max": 6.0},
    # RawDataPreprocessorMonocularDepth (tum.conf:633-640) and its IntensityFeatureExtractorBinned3D (tum.conf:858-883)
    "rgbd": {"depth_scaling_factor_to_meters": 0.001, "detector_threshold": 5, "enable_non_maximum_suppression": 1,
             "number_of_detectors_vertical": 3, "number_of_detectors_horizontal": 3, "target_number_of_keypoints": 1000},
}

CONFIGS = {"kitti": KITTI, "euroc": EUROC, "icl": ICL, "tum": TUM}


def _reentry(max_translation, min_inliers, min_inliers_ratio, max_chi_inliers):
    """MultiRelocalizer3D's own gates for re-entering an old local map (include/proslam_hip.h prs_reentry_params): the largest jump
    it attempts and its verdict thresholds -- not the loop detector's, which gate the closure itself (the "loop" groups above)"""
    return {"max_translation": max_translation, "relocalize_min_inliers": min_inliers, "relocalize_min_inliers_ratio": min_inliers_ratio,
            "relocalize_max_chi_inliers": max_chi_inliers}


REENTRY = {
    "kitti": _reentry(10, 25, 0.5, 5),       # kitti.conf:91-110: max_translation :100, chi :103, inliers :106, ratio :109
    "euroc": _reentry(2.5, 100, 0.9, 100),   # euroc.conf:134-153: :143, :146, :149, :152
    "icl": _reentry(3, 100, 0.5, 1000),      # icl.conf:687-706: :696, :699, :702, :705
    "tum": _reentry(1, 40, 0.5, 100),        # tum.conf:50-69: :59, :62, :65, :68
}


# the speckle filter behind dense stereo or in front of the dense cloud (include/proslam_hip.h prs_speckle_params; ops.speckle_params).
# BUILD-DEFINED: the reference has no dense images.  The values are the customary ones of OpenCV's StereoBM / StereoSGBM, a
# speckleWindowSize of 100 - 200 pixels and a speckleRange of 1 - 2 disparities: the larger window, the tighter range
SPECKLE = {"max_size": 200, "max_diff": 1.0}


# semi-global dense stereo (include/proslam_hip.h prs_sgm_stereo_params; ops.sgm_stereo_params).  BUILD-DEFINED: the reference has
# no dense matcher.  The penalties are on the scale of a 62-bit census cost: libSGM's defaults for its census costs, 10 and 120;
# eight paths, the uniqueness margin and the left-right tolerance of dense stereo
SGM_STEREO = {"n_disparities": 128, "min_disparity": 0, "p1": 10, "p2": 120, "n_paths": 8, "uniqueness_percent": 10, "lr_max_diff": 1}
# the bytes ops.SgmStereoBatch lets the S volumes of its workspace take when images_in_flight is left to it (the 26 bytes a pixel
# beside them grow with the batch whatever that count is).  2 GiB holds 17 KITTI-shaped images at 128 disparities (119 MB each): a
# path kernel's wave owns a line, and 17 x 376 rows are six waves for each of the 1024 SIMDs of an MI355X.  A constant, not a
# measurement
SGM_STEREO_VOLUME_BUDGET = 2 << 30


# the depth consistency filter between the speckle filter and the dense cloud (include/proslam_hip.h prs_depth_consistency_params;
# ops.depth_consistency_params).  BUILD-DEFINED: the reference has no dense images.  Two neighbours on each side, a depth agreeing
# within 2 % (COLMAP's geometric filter uses 1 %, on depths it has optimised jointly; a stereo depth is coarser), at least two
# neighbours in support and at most one that sees past the point; the ranges are the dense cloud's
DEPTH_CONSISTENCY = {"window": 2, "stride": 1, "max_rel_diff": 0.02, "min_support": 2, "max_violation": 1, "range_min": 0.1,
                     "range_max": 10.0}


# depth normals behind the dense cloud (include/proslam_hip_normals.h prs_depth_normals_params; ops.depth_normals_params).
# BUILD-DEFINED: the reference has no dense stage.  Neighbours two pixels out, a 3 x 3 smoothing window, and a depth edge where a
# neighbour's depth differs by more than 5 % of the centre's: the stereo depth of the matchers is quantised, so the gate is wider
# than the consistency filter's 2 %; the range is the dense cloud's.
DEPTH_NORMALS = {"radius": 2, "smooth": 1, "max_rel_diff": 0.05, "range_min": 0.1, "range_max": 10.0}


# TSDF fusion of the depth images (include/proslam_hip_tsdf.h prs_tsdf_params; ops.tsdf_params).  BUILD-DEFINED: the reference has
# no dense stage.  Voxels of 2 cm and a truncation of four voxels (KinectFusion's ratio: the band has to hold the depth noise and a
# few voxels on either side of the crossing for the normal), a weight that saturates at 64 observations so that the volume follows a
# scene that changes, every voxel seen once is surface; the range is the dense cloud's.
TSDF = {"voxel_size": 0.02, "truncation": 0.08, "max_weight": 64.0, "min_weight": 1.0, "range_min": 0.1, "range_max": 10.0}

# TSDF raycast of the fused volume (include/proslam_hip_tsdf_raycast.h prs_tsdf_raycast_params; ops.tsdf_raycast_params).
# BUILD-DEFINED.  A step of one default voxel, a quarter of the default truncation: a ray cannot cross the band between two samples;
# the weight threshold and the range are the fusion's.
TSDF_RAYCAST = {"step": 0.02, "min_weight": 1.0, "range_min": 0.1, "range_max": 10.0}

# dense frame-to-model aligner (include/proslam_hip_dense_align.h prs_dense_align_params; ops.dense_align_params).  BUILD-DEFINED.
# KinectFusion's gates in spirit: a pair is dropped when its points lie more than 20 cm apart or its normals more than about 37
# degrees; a point-to-plane residual beyond 10 cm is an outlier, down-weighted rather than dropped so that a coarse start still
# pulls; no damping; a step needs 100 inliers.  The schedule is (step, max_iterations) coarse to fine, KinectFusion's 4, 5, 10
# iterations on every fourth, every second and every pixel; the range is the dense cloud's.
DENSE_ALIGN = {"max_distance": 0.2, "min_normal_cos": 0.8, "robustifier": "saturated", "chi_threshold": 0.01, "damping": 0.0,
               "min_num_inliers": 100, "range_min": 0.1, "range_max": 10.0, "schedule": [(4, 4), (2, 5), (1, 10)]}


def _gate(mean_t, std_t, mean_r, std_r, where):
    return {"mean_translation": (mean_t,) * 3, "std_translation": (std_t,) * 3, "mean_rotation": (mean_r,) * 3,
            "std_rotation": (std_r,) * 3, "source": where}


# maximum_mean_translation_rmse, maximum_standard_deviation_translation_rmse (metres), maximum_mean_rotation_rmse,
# maximum_standard_deviation_rotation_rmse (degrees): the four Vector3f each benchmark program hands to isRegression
BENCHMARK_GATES = {
    "kitti": _gate(0.3, 1.0, 3, 3, "benchmarks/benchmark_kitti.cpp:17-20"),
    "icl": _gate(0.02, 0.1, 3, 3, "benchmarks/benchmark_icl.cpp:17-20"),
    "tum": _gate(0.05, 0.25, 3, 3, "benchmarks/benchmark_tum.cpp:17-20"),
    "euroc": _gate(0.5, 0.5, 3, 3, "benchmarks/benchmark_euroc.cpp:17-20"),
    "malaga": _gate(25, 10, 3, 3, "benchmarks/benchmark_malaga.cpp:17-20"),
}


def is_regression(result, gate):
    """True when a trajectory evaluator result (ops.TrajectoryEvalBatch.results) exceeds one of a benchmark's thresholds in any axis:
    axis_t_mean against mean_translation, axis_t_std against std_translation, axis_r_mean against mean_rotation, axis_r_std against
    std_rotation; also True for a result without relative poses or with an error status (nothing was measured).
    BUILD-DEFINED: the benchmark suite that owns isRegression and the statistics it compares is not in the reference tree.  The
    thresholds are the reference's; what they are compared with -- mean and population standard deviation of the absolute components
    of the relative pose error, metres and degrees -- is this build's reading of their names."""
    if isinstance(gate, str):
        gate = BENCHMARK_GATES[gate]
    if result["status"] < 0 or result["n_rpe"] < 1:
        return True
    pairs = (("axis_t_mean", "mean_translation"), ("axis_t_std", "std_translation"), ("axis_r_mean", "mean_rotation"),
             ("axis_r_std", "std_rotation"))
    return any(not (float(result[field][i]) <= gate[limit][i]) for field, limit in pairs for i in range(3))


def get(name):
    return copy.deepcopy(CONFIGS[name])


def baseline_pixels(cfg):
    """b_x = (K * t_right_in_left).x = fx * baseline (triangulator_rigid_stereo.cpp:105-106)"""
    return cfg["camera"]["fx"] * cfg["camera"]["baseline_m"]


def _selfcheck():
    assert abs(baseline_pixels(KITTI) - 386.1448) < 1e-3  # tests/fixtures.hpp:811
    assert math.isclose(_SQRT_FLT_MAX, math.sqrt(3.4028234663852886e38), rel_tol=1e-5)


_selfcheck()
