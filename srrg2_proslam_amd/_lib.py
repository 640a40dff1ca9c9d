"""ctypes loader for libproslam_hip.so (the HIP/gfx950 product library).

There is NO CPU fallback: if the shared library is missing or cannot be loaded, importing the
operators fails loudly.  Build it with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C srrg2_proslam_amd/csrc`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libproslam_hip.so")
ABI_VERSION = 104  # PRS_ABI_VERSION of include/proslam_hip.h

# status codes (include/proslam_hip.h)
OK = 0
WARN_EMPTY_INPUT = 1
WARN_NO_MATCHES = 2
WARN_LOW_RATIO = 4
WARN_RETRIED = 8
WARN_TRACK_LOST = 16
WARN_NO_PROJECTION = 32
WARN_SPARSE_DEPTH = 64  # PRS_WARN_SPARSE_DEPTH (RGB-D preprocessor)
ERR_NULL = -1
ERR_CAPACITY = -2
ERR_HIP = -3
ERR_RANGE = -4
ERR_UNSUPPORTED = -5
ERR_NO_DEVICE = -6
ERR_NOT_POSITIVE_DEFINITE = -10  # PRS_ERR_NOT_POSITIVE_DEFINITE (pose-graph optimiser)


class StereoParams(C.Structure):
    """prs_stereo_params"""
    _fields_ = [
        ("maximum_descriptor_distance", C.c_float),
        ("maximum_distance_ratio_to_second_best", C.c_float),
        ("minimum_matching_ratio", C.c_float),
        ("maximum_disparity_pixels", C.c_int32),
        ("epipolar_line_thickness_pixels", C.c_int32),
        ("image_rows", C.c_int32),
        ("image_cols", C.c_int32),
    ]


class TriangulatorParams(C.Structure):
    """prs_triangulator_params"""
    _fields_ = [
        ("fx", C.c_float),
        ("fy", C.c_float),
        ("cx", C.c_float),
        ("cy", C.c_float),
        ("b_x", C.c_float),
        ("minimum_disparity_pixels", C.c_float),
        ("infinity_depth_meters", C.c_float),
    ]


class StereoBatch(C.Structure):
    """prs_stereo_batch (device pointers)"""
    _fields_ = [
        ("batch", C.c_int32),
        ("stride", C.c_int32),
        ("left_kp", C.c_void_p),
        ("left_desc", C.c_void_p),
        ("n_left", C.c_void_p),
        ("right_kp", C.c_void_p),
        ("right_desc", C.c_void_p),
        ("n_right", C.c_void_p),
        ("matches", C.c_void_p),
        ("n_matches", C.c_void_p),
        ("status", C.c_void_p),
        ("fixed_uvuv", C.c_void_p),
        ("fixed_desc", C.c_void_p),
        ("n_fixed", C.c_void_p),
        ("fixed_xyz", C.c_void_p),
        ("triangulator", C.POINTER(TriangulatorParams)),
    ]


class Projector(C.Structure):
    """prs_projector"""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("canvas_cols", C.c_int32), ("canvas_rows", C.c_int32), ("range_min", C.c_float), ("range_max", C.c_float)]


class PcfParams(C.Structure):
    """prs_pcf_params"""
    _fields_ = [
        ("maximum_descriptor_distance", C.c_float),
        ("maximum_distance_ratio_to_second_best", C.c_float),
        ("minimum_matching_ratio", C.c_float),
        ("minimum_descriptor_distance", C.c_float),
        ("descriptor_distance_step_size_pixels", C.c_float),
        ("maximum_search_radius_pixels", C.c_uint64),
        ("minimum_search_radius_pixels", C.c_uint64),
        ("search_radius_step_size_pixels", C.c_uint64),
        ("minimum_number_of_iterations", C.c_uint64),
        ("maximum_estimate_change_norm_for_convergence", C.c_float),
        ("number_of_solver_iterations_per_projection", C.c_uint64),
        ("search_type", C.c_int32),
        ("projector", Projector),
        ("minimum_number_of_points_per_cluster", C.c_int32),  # KD-tree finder; 0 = the reference's default (10)
    ]


class PcfState(C.Structure):
    """prs_pcf_state"""
    _fields_ = [
        ("search_radius_pixels", C.c_uint64),
        ("current_iteration", C.c_uint64),
        ("descriptor_distance", C.c_float),
        ("has_converged", C.c_int32),
        ("config_changed", C.c_int32),
        ("num_recomputes", C.c_int32),
        ("local_map_in_sensor", C.c_float * 16),
        ("local_map_in_sensor_previous", C.c_float * 16),
        ("database_leaf_range", C.c_float),
        ("reserved", C.c_int32),
    ]


class AlignerParams(C.Structure):
    """prs_aligner_params"""
    _fields_ = [
        ("factor_type", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("image_cols", C.c_float), ("image_rows", C.c_float),
        ("baseline_left_in_right_px", C.c_float * 3),
        ("diagonal_info", C.c_float * 3),
        ("chi_threshold", C.c_float),
        ("enable_inverse_depth_weighting", C.c_int32),
        ("mean_disparity", C.c_float),
        ("damping", C.c_float),
        ("max_iterations", C.c_int32),
        ("min_num_inliers", C.c_int32),
        ("min_num_correspondences", C.c_int32),
        ("stop_at_fixed_point", C.c_int32),
        ("enable_inlier_only_runs", C.c_int32),
        ("keep_only_inlier_correspondences", C.c_int32),
        ("inlier_only_iterations", C.c_int32),
        ("with_sensor", C.c_int32),
        ("sensor_in_robot", C.c_float * 16),
        ("enable_motion_prior", C.c_int32),
        ("motion_prior_info", C.c_float * 6),
        ("kernel_weight_form", C.c_int32),       # 0 Omega / chi (shipped), 1 Omega * tau / chi
        ("damping_form", C.c_int32),             # 0 H + lambda diag(H) (shipped), 1 H + lambda I
        ("translation_weight_form", C.c_int32),  # 0 min(0.01 + dn, 1) (shipped), 1 clamp(dn, 0.01, 1)
        ("step_norm_exit", C.c_float),           # opt-in early exit (less work than the reference); 0 = off
    ]


class AlignResult(C.Structure):
    """prs_align_result"""
    _fields_ = [
        ("H", C.c_float * 36),
        ("b", C.c_float * 6),
        ("chi_inliers", C.c_float),
        ("chi_total", C.c_float),
        ("mean_disparity", C.c_float),
        ("num_inliers", C.c_int32),
        ("num_outliers", C.c_int32),
        ("num_invalid", C.c_int32),
        ("num_correspondences", C.c_int32),
        ("status", C.c_int32),
        ("iterations", C.c_int32),
        ("iterations_executed", C.c_int32),
        ("warnings", C.c_int32),
    ]


class AlignBatch(C.Structure):
    """prs_align_batch (device pointers)"""
    _fields_ = [
        ("batch", C.c_int32), ("fixed_stride", C.c_int32), ("moving_stride", C.c_int32),
        ("fixed", C.c_void_p), ("fixed_desc", C.c_void_p), ("n_fixed", C.c_void_p),
        ("moving", C.c_void_p), ("moving_desc", C.c_void_p), ("n_moving", C.c_void_p),
        ("inputs_changed", C.c_void_p), ("state", C.c_void_p), ("X", C.c_void_p),
        ("corr", C.c_void_p), ("n_corr", C.c_void_p), ("result", C.c_void_p), ("prior", C.c_void_p),
        ("prior_mean", C.c_void_p), ("max_fixed", C.c_int32),
    ]


class ClipBatch(C.Structure):
    """prs_clip_batch (device pointers)"""
    _fields_ = [
        ("batch", C.c_int32), ("stride", C.c_int32),
        ("scene_xyzw", C.c_void_p), ("scene_desc", C.c_void_p), ("n_scene", C.c_void_p),
        ("robot_in_local_map", C.c_void_p),
        ("clipped_xyzw", C.c_void_p), ("clipped_desc", C.c_void_p), ("global_indices", C.c_void_p),
        ("n_clipped", C.c_void_p), ("status", C.c_void_p), ("scene_n_opt", C.c_void_p),
    ]


class BruteforceParams(C.Structure):
    """prs_bruteforce_params"""
    _fields_ = [
        ("maximum_descriptor_distance", C.c_float),
        ("maximum_distance_ratio_to_second_best", C.c_float),
        ("minimum_matching_ratio", C.c_float),
    ]


class BruteforceBatch(C.Structure):
    """prs_bruteforce_batch (device pointers)"""
    _fields_ = [
        ("batch", C.c_int32), ("fixed_stride", C.c_int32), ("moving_stride", C.c_int32),
        ("fixed_desc", C.c_void_p), ("n_fixed", C.c_void_p), ("moving_desc", C.c_void_p), ("n_moving", C.c_void_p),
        ("matches", C.c_void_p), ("n_matches", C.c_void_p), ("status", C.c_void_p),
        ("candidate_capacity", C.c_int32),
    ]


class EstimatorParams(C.Structure):
    """prs_estimator_params"""
    _fields_ = [("type", C.c_int32), ("measurement_dim", C.c_int32),
                ("maximum_distance_geometry_meters_squared", C.c_float),
                ("minimum_state_element_covariance", C.c_double), ("maximum_covariance_norm_squared", C.c_double),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("b_x", C.c_double), ("b_y", C.c_double),
                ("maximum_number_of_iterations", C.c_uint32), ("convergence_criterion_minimum_chi2_delta", C.c_float),
                ("maximum_reprojection_error_pixels_squared", C.c_float),
                ("minimum_number_of_measurements_for_optimization", C.c_uint32),
                ("camera_matrix", C.c_float * 9)]


class MergerParams(C.Structure):
    """prs_merger_params"""
    _fields_ = [("variant", C.c_int32), ("enable_binning", C.c_int32),
                ("number_of_row_bins", C.c_uint32), ("number_of_col_bins", C.c_uint32),
                ("canvas_rows", C.c_int32), ("canvas_cols", C.c_int32),
                ("maximum_distance_appearance", C.c_float), ("target_number_of_merges", C.c_uint32),
                ("target_merge_ratio", C.c_float), ("triangulator", TriangulatorParams),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("estimator", EstimatorParams)]


class MergeResult(C.Structure):
    """prs_merge_result"""
    _fields_ = [("n_merged", C.c_int32), ("n_added", C.c_int32), ("status", C.c_int32)]


class MergeBatch(C.Structure):
    """prs_merge_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("capacity", C.c_int32), ("max_measurements", C.c_int32), ("max_frames", C.c_int32),
                ("coords", C.c_void_p), ("desc", C.c_void_p), ("state", C.c_void_p), ("covariance", C.c_void_p),
                ("n_opt", C.c_void_p), ("inlier", C.c_void_p), ("n_meas", C.c_void_p), ("meas", C.c_void_p),
                ("poses", C.c_void_p), ("n_points", C.c_void_p),
                ("measurement_stride", C.c_int32), ("measurement", C.c_void_p), ("measurement_desc", C.c_void_p),
                ("n_measured", C.c_void_p), ("corr_stride", C.c_int32), ("corr", C.c_void_p), ("n_corr", C.c_void_p),
                ("scene_index_map", C.c_void_p), ("measurement_in_world", C.c_void_p), ("measurement_in_scene", C.c_void_p),
                ("frame", C.c_void_p), ("result", C.c_void_p), ("corr_from_aligner", C.c_int32)]


class ExtractorParams(C.Structure):
    """prs_extractor_params"""
    _fields_ = [("detector_threshold", C.c_int32), ("enable_non_maximum_suppression", C.c_int32),
                ("target_number_of_keypoints", C.c_int32), ("number_of_detectors_vertical", C.c_int32),
                ("number_of_detectors_horizontal", C.c_int32), ("selection_order", C.c_int32),
                ("max_raw_detections", C.c_int32)]


class ExtractBatch(C.Structure):
    """prs_extract_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("pitch", C.c_int32), ("images", C.c_void_p),
                ("stride", C.c_int32), ("keypoints", C.c_void_p), ("intensity", C.c_void_p), ("descriptors", C.c_void_p),
                ("n_features", C.c_void_p), ("status", C.c_void_p)]


class SelectiveExtractorParams(C.Structure):
    """prs_selective_extractor_params"""
    _fields_ = [("detector_type", C.c_int32), ("descriptor_type", C.c_int32), ("target_number_of_keypoints", C.c_int32),
                ("target_bin_width_pixels", C.c_int32), ("enable_full_distance_to_left", C.c_int32),
                ("enable_full_distance_to_right", C.c_int32), ("enable_seeding_when_tracking", C.c_int32),
                ("max_candidates", C.c_int32)]


class SelectiveExtractBatch(C.Structure):
    """prs_selective_extract_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("pitch", C.c_int32), ("images", C.c_void_p),
                ("projection_stride", C.c_int32), ("projections", C.c_void_p), ("n_projections", C.c_void_p),
                ("detection_radius", C.c_void_p), ("seeding_mask", C.c_void_p), ("stride", C.c_int32), ("keypoints", C.c_void_p),
                ("intensity", C.c_void_p), ("descriptors", C.c_void_p), ("n_features", C.c_void_p), ("status", C.c_void_p)]


class DepthParams(C.Structure):
    """prs_depth_params"""
    _fields_ = [("depth_type", C.c_int32), ("depth_scaling_factor_to_meters", C.c_float)]


class DepthBatch(C.Structure):
    """prs_depth_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("pitch", C.c_int32), ("depth", C.c_void_p),
                ("stride", C.c_int32), ("keypoints", C.c_void_p), ("intensity", C.c_void_p), ("descriptors", C.c_void_p),
                ("n_features", C.c_void_p), ("extract_status", C.c_void_p), ("fixed", C.c_void_p), ("fixed_desc", C.c_void_p),
                ("fixed_intensity", C.c_void_p), ("n_fixed", C.c_void_p), ("status", C.c_void_p)]


ROBUSTIFIER_CLAMP, ROBUSTIFIER_SATURATED = 0, 1  # PRS_ROBUSTIFIER_*


class PointAlignParams(C.Structure):
    """prs_point_align_params"""
    _fields_ = [("robustifier", C.c_int32), ("chi_threshold", C.c_float), ("damping", C.c_float), ("max_iterations", C.c_int32),
                ("min_num_inliers", C.c_int32), ("min_num_correspondences", C.c_int32), ("relocalize_min_inliers", C.c_int32),
                ("relocalize_min_inliers_ratio", C.c_float), ("relocalize_max_chi_inliers", C.c_float), ("linearize_only", C.c_int32),
                ("parked_per_lane", C.c_int32)]


class PointAlignResult(C.Structure):
    """prs_point_align_result"""
    _fields_ = [("H", C.c_float * 36), ("b", C.c_float * 6), ("chi_inliers", C.c_float), ("chi_total", C.c_float),
                ("num_inliers", C.c_int32), ("num_outliers", C.c_int32), ("num_invalid", C.c_int32), ("num_correspondences", C.c_int32),
                ("status", C.c_int32), ("accepted", C.c_int32), ("iterations", C.c_int32), ("warnings", C.c_int32)]


class PointAlignPairs(C.Structure):
    """prs_point_align_pairs (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("fixed_stride", C.c_int32), ("moving_stride", C.c_int32), ("corr_stride", C.c_int32),
                ("fixed", C.c_void_p), ("n_fixed", C.c_void_p), ("moving", C.c_void_p), ("n_moving", C.c_void_p), ("corr", C.c_void_p),
                ("n_corr", C.c_void_p), ("match_status", C.c_void_p), ("X", C.c_void_p), ("result", C.c_void_p),
                ("inlier_mask", C.c_void_p)]


class PlaceParams(C.Structure):
    """prs_place_params"""
    _fields_ = [("maximum_descriptor_distance", C.c_float), ("minimum_age_difference_to_candidates", C.c_uint32),
                ("relocalize_min_inliers", C.c_int32), ("max_candidates", C.c_int32)]


class PlaceQueries(C.Structure):
    """prs_place_queries (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("query_stride", C.c_int32), ("desc", C.c_void_p), ("valid", C.c_void_p), ("xyz", C.c_void_p),
                ("n_query", C.c_void_p), ("graph_id", C.c_void_p), ("count_stride", C.c_int32), ("match_counts", C.c_void_p),
                ("key_stride", C.c_int32), ("best_keys", C.c_void_p), ("corr_stride", C.c_int32), ("candidates", C.c_void_p),
                ("n_candidates", C.c_void_p), ("corr", C.c_void_p), ("n_corr", C.c_void_p), ("status", C.c_void_p),
                ("index_query", C.c_void_p)]


class PlacePairs(C.Structure):
    """prs_place_pairs (device pointers)"""
    _fields_ = [("fixed_stride", C.c_int32), ("moving_stride", C.c_int32), ("fixed_xyz", C.c_void_p), ("fixed_desc", C.c_void_p),
                ("n_fixed", C.c_void_p), ("moving_xyz", C.c_void_p), ("moving_desc", C.c_void_p), ("n_moving", C.c_void_p),
                ("X", C.c_void_p)]


class PlaceBankAppend(C.Structure):
    """prs_place_bank_append (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("query_stride", C.c_int32), ("desc", C.c_void_p), ("valid", C.c_void_p), ("xyz", C.c_void_p),
                ("n_query", C.c_void_p), ("graph_id", C.c_void_p), ("graph_id_base", C.c_void_p), ("status", C.c_void_p)]


class PlaceBankLinks(C.Structure):
    """prs_place_bank_links (device pointers)"""
    _fields_ = [("candidates_flat", C.c_void_p), ("query_node", C.c_void_p), ("graph_id_base", C.c_void_p)]


DAMPING_DIAG, DAMPING_IDENTITY = 0, 1  # PRS_DAMPING_*
POSE_GRAPH_MAX_ITERATIONS = 32         # PRS_POSE_GRAPH_MAX_ITERATIONS


class PoseGraphParams(C.Structure):
    """prs_pose_graph_params"""
    _fields_ = [("damping", C.c_float), ("damping_form", C.c_int32), ("max_iterations", C.c_int32), ("epsilon", C.c_float),
                ("closure_information", C.c_float)]


class PoseGraphResult(C.Structure):
    """prs_pose_graph_result"""
    _fields_ = [("chi", C.c_double * POSE_GRAPH_MAX_ITERATIONS), ("chi_final", C.c_double), ("linearizations", C.c_int32),
                ("iterations", C.c_int32), ("envelope_blocks", C.c_int32), ("status", C.c_int32)]


class PoseGraphLmParams(C.Structure):
    """prs_pose_graph_lm_params"""
    _fields_ = [("user_lambda_init", C.c_float), ("tau", C.c_float), ("step_high", C.c_float), ("step_low", C.c_float),
                ("lm_iterations_max", C.c_int32), ("variable_damping", C.c_int32), ("max_iterations", C.c_int32), ("epsilon", C.c_float)]


class PoseGraphLmResult(C.Structure):
    """prs_pose_graph_lm_result"""
    _fields_ = [("chi", C.c_double * POSE_GRAPH_MAX_ITERATIONS), ("chi_final", C.c_double), ("lambda_", C.c_double * POSE_GRAPH_MAX_ITERATIONS),
                ("trials", C.c_int32 * POSE_GRAPH_MAX_ITERATIONS), ("linearizations", C.c_int32), ("iterations", C.c_int32),
                ("envelope_blocks", C.c_int32), ("status", C.c_int32), ("trials_total", C.c_int32),
                ("rejected_not_positive_definite", C.c_int32), ("stalled", C.c_int32), ("reserved", C.c_int32)]


class PoseGraphs(C.Structure):
    """prs_pose_graphs (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("node_stride", C.c_int32), ("edge_stride", C.c_int32), ("reserved", C.c_int32),
                ("X", C.c_void_p), ("fixed", C.c_void_p), ("n_nodes", C.c_void_p), ("from_", C.c_void_p), ("to", C.c_void_p),
                ("Z", C.c_void_p), ("omega", C.c_void_p), ("n_edges", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_uint64), ("result", C.c_void_p)]


class PoseGraphClosures(C.Structure):
    """prs_pose_graph_closures (device pointers)"""
    _fields_ = [("n_queries", C.c_int32), ("max_candidates", C.c_int32), ("n_maps", C.c_int32), ("reserved", C.c_int32),
                ("candidates", C.c_void_p), ("result", C.c_void_p), ("X", C.c_void_p), ("graph_of_query", C.c_void_p),
                ("node_of_query", C.c_void_p), ("node_of_map", C.c_void_p), ("status", C.c_void_p), ("n_appended", C.c_void_p)]


CLOSURE_XYZ, CLOSURE_UVD = 0, 1  # PRS_CLOSURE_*


class ClosureMergerParams(C.Structure):
    """prs_closure_merger_params"""
    _fields_ = [("measurement_kind", C.c_int32), ("enable_binning", C.c_int32), ("number_of_row_bins", C.c_uint32),
                ("number_of_col_bins", C.c_uint32), ("canvas_rows", C.c_int32), ("canvas_cols", C.c_int32), ("fx", C.c_float),
                ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("maximum_distance_geometry_squared", C.c_float),
                ("maximum_response", C.c_float), ("target_number_of_merges", C.c_uint32)]


class ClosureMergeBatch(C.Structure):
    """prs_closure_merge_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("capacity", C.c_int32), ("coords", C.c_void_p), ("desc", C.c_void_p), ("n_points", C.c_void_p),
                ("state", C.c_void_p), ("covariance", C.c_void_p), ("n_opt", C.c_void_p), ("inlier", C.c_void_p), ("n_meas", C.c_void_p),
                ("scene_in_world", C.c_void_p), ("measurement_stride", C.c_int32), ("corr_stride", C.c_int32),
                ("measurement", C.c_void_p), ("measurement_desc", C.c_void_p), ("n_measured", C.c_void_p), ("corr", C.c_void_p),
                ("n_corr", C.c_void_p), ("transform", C.c_void_p), ("gate", C.c_void_p), ("result", C.c_void_p),
                ("corr_from_aligner", C.c_int32), ("transform_is_scene_in_measurement", C.c_int32)]


SESSION_NO_SPLIT, SESSION_SPLIT_VIEWPOINT, SESSION_SPLIT_LOST = 0, 1, 2  # PRS_SESSION_*


class SessionParams(C.Structure):
    """prs_session_params"""
    _fields_ = [("local_map_distance", C.c_float), ("local_map_angle_distance_radians", C.c_float), ("split_information", C.c_float),
                ("lost_information", C.c_float)]


class SessionBatch(C.Structure):
    """prs_session_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("frame_stride", C.c_int32), ("capacity", C.c_int32), ("node_stride", C.c_int32),
                ("edge_stride", C.c_int32), ("handover_stride", C.c_int32),
                ("pose", C.c_void_p), ("prev", C.c_void_p), ("prediction", C.c_void_p), ("slot", C.c_void_p), ("cur_node", C.c_void_p),
                ("n_frames", C.c_void_p), ("frame_node", C.c_void_p), ("frame_pose", C.c_void_p), ("status", C.c_void_p),
                ("reason", C.c_void_p), ("X", C.c_void_p), ("result", C.c_void_p), ("n_corr", C.c_void_p), ("coords", C.c_void_p),
                ("desc", C.c_void_p), ("n_points", C.c_void_p), ("n_meas", C.c_void_p), ("frame", C.c_void_p),
                ("n_corr_merge", C.c_void_p), ("measurement_in_world", C.c_void_p), ("measurement_in_scene", C.c_void_p),
                ("graph_X", C.c_void_p), ("fixed", C.c_void_p), ("n_nodes", C.c_void_p), ("from_", C.c_void_p), ("to", C.c_void_p),
                ("Z", C.c_void_p), ("omega", C.c_void_p), ("n_edges", C.c_void_p), ("handover_desc", C.c_void_p),
                ("handover_xyz", C.c_void_p), ("handover_n_query", C.c_void_p), ("handover_graph_id", C.c_void_p),
                ("graph_id_base", C.c_void_p)]


class MapArchive(C.Structure):
    """prs_map_archive (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("capacity", C.c_int32), ("slot_stride", C.c_int32), ("node_stride", C.c_int32),
                ("max_measurements", C.c_int32), ("max_frames", C.c_int32),
                ("coords", C.c_void_p), ("desc", C.c_void_p), ("state", C.c_void_p), ("covariance", C.c_void_p), ("n_opt", C.c_void_p),
                ("inlier", C.c_void_p), ("n_meas", C.c_void_p), ("n_points", C.c_void_p), ("next_frame", C.c_void_p),
                ("meas", C.c_void_p), ("poses", C.c_void_p), ("slot_of_node", C.c_void_p), ("n_slots", C.c_void_p), ("status", C.c_void_p)]


class ReentryParams(C.Structure):
    """prs_reentry_params"""
    _fields_ = [("max_translation", C.c_float), ("relocalize_min_inliers", C.c_int32), ("relocalize_min_inliers_ratio", C.c_float),
                ("relocalize_max_chi_inliers", C.c_float)]


class ReentryBatch(C.Structure):
    """prs_reentry_batch (device pointers)"""
    _fields_ = [("max_candidates", C.c_int32), ("map_stride", C.c_int32), ("corr_stride", C.c_int32), ("reserved", C.c_int32),
                ("candidates_flat", C.c_void_p), ("result", C.c_void_p), ("X", C.c_void_p), ("corr", C.c_void_p), ("n_corr", C.c_void_p),
                ("node_of_map", C.c_void_p), ("n_measured", C.c_void_p), ("reentered", C.c_void_p), ("status", C.c_void_p),
                ("merge_corr", C.c_void_p), ("merge_n_corr", C.c_void_p), ("merge_transform", C.c_void_p),
                ("scene_in_world", C.c_void_p), ("gate", C.c_void_p)]


TRAJ_ALIGN_NONE, TRAJ_ALIGN_FIRST, TRAJ_ALIGN_RIGID = 0, 1, 2  # PRS_TRAJ_ALIGN_*


class TrajectoryParams(C.Structure):
    """prs_trajectory_params"""
    _fields_ = [("align", C.c_int32), ("rpe_delta", C.c_int32), ("kitti_step", C.c_int32), ("n_lengths", C.c_int32),
                ("lengths", C.c_float * 8)]


class TrajectoryResult(C.Structure):
    """prs_trajectory_result"""
    _fields_ = [("status", C.c_int32), ("n_valid", C.c_int32), ("n_rpe", C.c_int32), ("n_kitti", C.c_int32), ("S", C.c_double * 16),
                ("path_length", C.c_double), ("ate_rmse", C.c_double), ("ate_mean", C.c_double), ("ate_max", C.c_double),
                ("rpe_t_rmse", C.c_double), ("rpe_t_mean", C.c_double), ("rpe_t_max", C.c_double),
                ("rpe_r_rmse", C.c_double), ("rpe_r_mean", C.c_double), ("rpe_r_max", C.c_double),
                ("axis_t_mean", C.c_double * 3), ("axis_t_std", C.c_double * 3), ("axis_r_mean", C.c_double * 3),
                ("axis_r_std", C.c_double * 3), ("kitti_t", C.c_double), ("kitti_r", C.c_double), ("kitti_t_len", C.c_double * 8),
                ("kitti_r_len", C.c_double * 8), ("kitti_n_len", C.c_int32 * 8)]


class TrajectoryBatch(C.Structure):
    """prs_trajectory_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("frame_stride", C.c_int32), ("estimate", C.c_void_p), ("ground_truth", C.c_void_p),
                ("n_frames", C.c_void_p), ("valid", C.c_void_p), ("result", C.c_void_p), ("frame_error", C.c_void_p),
                ("workspace", C.c_void_p)]


class WorldMapParams(C.Structure):
    """prs_world_map_params"""
    _fields_ = [("min_n_opt", C.c_uint32), ("require_inlier", C.c_int32), ("include_live", C.c_int32), ("refresh_state", C.c_int32)]


class WorldMapBatch(C.Structure):
    """prs_world_map_batch (device pointers)"""
    _fields_ = [("out_stride", C.c_int32), ("reserved", C.c_int32), ("xyz", C.c_void_p), ("desc", C.c_void_p), ("node", C.c_void_p),
                ("row", C.c_void_p), ("n_opt", C.c_void_p), ("n_out", C.c_void_p), ("n_total", C.c_void_p), ("n_nonfinite", C.c_void_p),
                ("bounds", C.c_void_p), ("status", C.c_void_p), ("workspace", C.c_void_p)]


class WorldVoxelParams(C.Structure):
    """prs_world_voxel_params"""
    _fields_ = [("voxel_size", C.c_float), ("position", C.c_int32), ("reserved", C.c_int32 * 2)]


class WorldVoxelBatch(C.Structure):
    """prs_world_voxel_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("in_stride", C.c_int32), ("in_xyz", C.c_void_p), ("in_n", C.c_void_p), ("in_n_opt", C.c_void_p),
                ("in_desc", C.c_void_p), ("in_node", C.c_void_p), ("in_row", C.c_void_p), ("out_stride", C.c_int32),
                ("table_stride", C.c_int32), ("xyz", C.c_void_p), ("index", C.c_void_p), ("count", C.c_void_p), ("desc", C.c_void_p),
                ("node", C.c_void_p), ("row", C.c_void_p), ("n_opt", C.c_void_p), ("n_out", C.c_void_p), ("n_voxels", C.c_void_p),
                ("n_nonfinite", C.c_void_p), ("n_outside", C.c_void_p), ("status", C.c_void_p), ("workspace", C.c_void_p)]


class RectifyMap(C.Structure):
    """prs_rectify_map: one camera's map, an element of a device array (96 bytes)"""
    _fields_ = [("model", C.c_int32), ("reserved", C.c_int32), ("src_fx", C.c_float), ("src_fy", C.c_float), ("src_cx", C.c_float),
                ("src_cy", C.c_float), ("k1", C.c_float), ("k2", C.c_float), ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float),
                ("R", C.c_float * 9), ("dst_fx", C.c_float), ("dst_fy", C.c_float), ("dst_cx", C.c_float), ("dst_cy", C.c_float)]


class RectifyParams(C.Structure):
    """prs_rectify_params"""
    _fields_ = [("pixel_type", C.c_int32), ("interpolation", C.c_int32), ("border", C.c_float), ("reserved", C.c_int32)]


class RectifyBatch(C.Structure):
    """prs_rectify_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("src_rows", C.c_int32), ("src_cols", C.c_int32), ("src_pitch", C.c_int32), ("src", C.c_void_p),
                ("dst_rows", C.c_int32), ("dst_cols", C.c_int32), ("dst_pitch", C.c_int32), ("dst", C.c_void_p), ("n_maps", C.c_int32),
                ("maps", C.c_void_p), ("map_of", C.c_void_p), ("n_border", C.c_void_p), ("status", C.c_void_p)]


class DepthCloudParams(C.Structure):
    """prs_depth_cloud_params"""
    _fields_ = [("depth_type", C.c_int32), ("depth_scaling_factor_to_meters", C.c_float), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("range_min", C.c_float), ("range_max", C.c_float), ("step", C.c_int32),
                ("sensor_in_robot", C.c_float * 16), ("reserved", C.c_int32 * 3)]


class DepthCloudBatch(C.Structure):
    """prs_depth_cloud_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("frames", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("pitch", C.c_int32),
                ("gray_pitch", C.c_int32), ("pose_stride", C.c_int32), ("out_stride", C.c_int32), ("depth", C.c_void_p), ("gray", C.c_void_p),
                ("n_images", C.c_void_p), ("pose", C.c_void_p), ("frame_index", C.c_void_p), ("n_base", C.c_void_p), ("xyz", C.c_void_p),
                ("frame", C.c_void_p), ("pixel", C.c_void_p), ("n_out", C.c_void_p), ("n_total", C.c_void_p), ("n_skipped", C.c_void_p),
                ("status", C.c_void_p), ("workspace", C.c_void_p)]


class DenseStereoParams(C.Structure):
    """prs_dense_stereo_params"""
    _fields_ = [("n_disparities", C.c_int32), ("min_disparity", C.c_int32), ("aggregation_radius", C.c_int32),
                ("uniqueness_percent", C.c_int32), ("lr_max_diff", C.c_int32), ("bf", C.c_float), ("reserved", C.c_int32 * 6)]


class DenseStereoBatch(C.Structure):
    """prs_dense_stereo_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("frames", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("left_pitch", C.c_int32),
                ("right_pitch", C.c_int32), ("out_pitch", C.c_int32), ("reserved0", C.c_int32), ("left", C.c_void_p), ("right", C.c_void_p),
                ("n_images", C.c_void_p), ("disparity", C.c_void_p), ("depth", C.c_void_p), ("n_valid", C.c_void_p), ("status", C.c_void_p),
                ("workspace", C.c_void_p)]


class SpeckleParams(C.Structure):
    """prs_speckle_params"""
    _fields_ = [("pixel_type", C.c_int32), ("companion_type", C.c_int32), ("max_diff", C.c_float), ("max_size", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class SpeckleBatch(C.Structure):
    """prs_speckle_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("frames", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("pitch", C.c_int32),
                ("companion_pitch", C.c_int32), ("label_pitch", C.c_int32), ("reserved0", C.c_int32), ("image", C.c_void_p),
                ("companion", C.c_void_p), ("n_images", C.c_void_p), ("label", C.c_void_p), ("n_kept", C.c_void_p), ("n_removed", C.c_void_p),
                ("status", C.c_void_p), ("workspace", C.c_void_p)]


class SgmStereoParams(C.Structure):
    """prs_sgm_stereo_params"""
    _fields_ = [("n_disparities", C.c_int32), ("min_disparity", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("n_paths", C.c_int32),
                ("uniqueness_percent", C.c_int32), ("lr_max_diff", C.c_int32), ("bf", C.c_float), ("reserved", C.c_int32 * 4)]


class SgmStereoBatch(C.Structure):
    """prs_sgm_stereo_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("frames", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("left_pitch", C.c_int32),
                ("right_pitch", C.c_int32), ("out_pitch", C.c_int32), ("images_in_flight", C.c_int32), ("left", C.c_void_p),
                ("right", C.c_void_p), ("n_images", C.c_void_p), ("disparity", C.c_void_p), ("depth", C.c_void_p), ("n_valid", C.c_void_p),
                ("status", C.c_void_p), ("workspace", C.c_void_p)]


class DepthConsistencyParams(C.Structure):
    """prs_depth_consistency_params"""
    _fields_ = [("depth_type", C.c_int32), ("depth_scaling_factor_to_meters", C.c_float), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("range_min", C.c_float), ("range_max", C.c_float), ("window", C.c_int32),
                ("stride", C.c_int32), ("max_rel_diff", C.c_float), ("min_support", C.c_int32), ("max_violation", C.c_int32),
                ("sensor_in_robot", C.c_float * 16), ("reserved", C.c_int32 * 3)]


class DepthConsistencyBatch(C.Structure):
    """prs_depth_consistency_batch (device pointers)"""
    _fields_ = [("batch", C.c_int32), ("frames", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("pitch", C.c_int32),
                ("out_pitch", C.c_int32), ("count_pitch", C.c_int32), ("pose_stride", C.c_int32), ("depth", C.c_void_p),
                ("n_images", C.c_void_p), ("pose", C.c_void_p), ("frame_index", C.c_void_p), ("out", C.c_void_p), ("support", C.c_void_p),
                ("violation", C.c_void_p), ("n_kept", C.c_void_p), ("n_removed", C.c_void_p), ("n_skipped", C.c_void_p),
                ("status", C.c_void_p), ("workspace", C.c_void_p)]


class DispatchEnv(C.Structure):
    """prs_dispatch_env: what a dispatch depends on outside its arguments (tests and tools)"""
    _fields_ = [(n, C.c_int32) for n in ("cus", "fused_align", "matcher_v3", "force_unstaged", "no_lone_gn", "merge_fused", "bf_mfma", "stamps",
                                         "stamps_split", "bf_global_state", "bf_two_workgroups", "no_search_reuse")]


class PlanLaunch(C.Structure):
    """prs_plan_launch"""
    _fields_ = [("kernel", C.c_char_p), ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("block", C.c_int32), ("lds_bytes", C.c_uint32)]


class DispatchPlan(C.Structure):
    """prs_dispatch_plan"""
    _fields_ = [("status", C.c_int32), ("message", C.c_char_p), ("n_launches", C.c_int32), ("launch", PlanLaunch * 4), ("fact", C.c_int32 * 48)]


class GuardExtent(C.Structure):
    """prs_guard_extent: what prs_guard_layout answers"""
    _fields_ = [("total", C.c_uint64), ("user_offset", C.c_uint64), ("tail_bytes", C.c_uint64)]


class GuardRegion(C.Structure):
    """prs_guard_region: a live block of a context in guard mode"""
    _fields_ = [("user", C.c_void_p), ("bytes", C.c_uint64), ("tail_bytes", C.c_uint64), ("pinned", C.c_int32), ("reserved", C.c_int32),
                ("name", C.c_char * 48)]


GUARD_SLACK_EXACT, GUARD_SLACK_QUARTER, GUARD_SLACK_HALF = 0, 1, 2
GUARD_BAND, GUARD_PATTERN = 4096, 0xA5

DISPATCH_STEREO, DISPATCH_ALIGN, DISPATCH_BRUTEFORCE, DISPATCH_MERGE = 0, 1, 2, 3
# the PRS_PLAN_<FAMILY>_* enumerators in order, lower case
PLAN_FACTS = {
    DISPATCH_STEREO: ("v5", "v5_why", "cap", "off_pool", "pool_cap", "v5_lds", "kpt", "epi", "stage", "staged_lds", "unstaged_lds", "sort_cap",
                      "best_lim"),
    DISPATCH_ALIGN: ("max_fixed", "cell_sy", "cell_sx", "cell_ncy", "cell_ncx", "lut_cap", "split", "surv_slots", "db_blob", "lone", "five",
                     "fast", "plain", "mprior", "depth", "off_u", "search_off_u"),
    DISPATCH_BRUTEFORCE: ("lim", "nw", "cap", "grid", "chunks", "bm_fits", "lvl_cap", "fused_matrix", "dual", "mfma", "lds", "off_cnt_f",
                          "off_cnt_m", "off_reg_f", "off_reg_m", "off_acc", "off_hist", "off_bm", "off_lvl", "off_mx"),
    DISPATCH_MERGE: ("nbr", "nbc", "split", "off_owner", "off_first", "off_best", "off_seen", "off_sh", "off_wave", "off_pose_cache",
                     "tail_capacity"),
}

MODE_ALIGN, MODE_FINDER, MODE_LINEARIZE = 0, 1, 2

# every symbol include/proslam_hip.h declares: (restype, argtypes)
_vp = C.c_void_p
_i32p = C.POINTER(C.c_int32)
SYMBOLS = {
    "prs_version": (C.c_int, []),
    "prs_launch_fits": (C.c_int, [C.c_int64, C.c_int32]),
    "prs_guard_layout": (C.c_int, [C.c_uint64, C.c_int32, C.c_int32, C.POINTER(GuardExtent)]),
    "prs_context_guard_check": (C.c_int, [_vp, C.c_char_p, C.c_uint64]),
    "prs_context_guard_regions": (C.c_int, [_vp, C.POINTER(GuardRegion), C.c_int32]),
    "prs_guard_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_abi_check": (C.c_int, [C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]),
    "prs_status_string": (C.c_char_p, [C.c_int]),
    "prs_context_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "prs_context_destroy": (C.c_int, [_vp]),
    "prs_context_set_stream": (C.c_int, [_vp, _vp]),
    "prs_context_use_own_stream": (C.c_int, [_vp]),
    "prs_context_synchronize": (C.c_int, [_vp]),
    "prs_context_enable_timing": (C.c_int, [_vp, C.c_int32]),
    "prs_context_set_bruteforce_dense_phase": (C.c_int, [_vp, C.c_int32]),
    "prs_context_get_align_timing": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "prs_context_get_align_round_timing": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "prs_context_get_search_reuse": (C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "prs_last_error": (C.c_char_p, [_vp]),
    "prs_stereo_match": (C.c_int, [_vp, C.POINTER(StereoParams), _vp, _vp, C.c_int32, _vp, _vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "prs_stereo_match_batch": (C.c_int, [_vp, C.POINTER(StereoParams), C.POINTER(StereoBatch)]),
    "prs_align_batch_run": (C.c_int, [_vp, C.POINTER(PcfParams), C.POINTER(AlignerParams), C.POINTER(AlignBatch), C.c_int32]),
    "prs_align_batch_enqueue": (C.c_int, [_vp, C.POINTER(PcfParams), C.POINTER(AlignerParams), C.POINTER(AlignBatch), C.c_int32]),
    "prs_align_batch_finish": (C.c_int, [_vp]),
    "prs_align_batch_rearm": (C.c_int, [_vp]),
    "prs_align_batch_rearm_on": (C.c_int, [_vp, _vp]),
    "prs_pcf_create": (C.c_int, [_vp, C.POINTER(PcfParams), C.POINTER(_vp)]),
    "prs_pcf_destroy": (C.c_int, [_vp]),
    "prs_pcf_set_params": (C.c_int, [_vp, C.POINTER(PcfParams)]),
    "prs_pcf_set_fixed": (C.c_int, [_vp, _vp, C.c_int32, _vp, C.c_int32]),
    "prs_pcf_set_moving": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32]),
    "prs_pcf_set_local_map_in_sensor": (C.c_int, [_vp, _vp]),
    "prs_pcf_set_search_radius": (C.c_int, [_vp, C.c_uint64]),
    "prs_pcf_set_descriptor_distance": (C.c_int, [_vp, C.c_float]),
    "prs_pcf_get_state": (C.c_int, [_vp, C.POINTER(PcfState)]),
    "prs_pcf_set_motion_prior_mean": (C.c_int, [_vp, _vp]),
    "prs_pcf_compute": (C.c_int, [_vp, _vp, C.c_int32, _i32p]),
    "prs_pcf_align": (C.c_int, [_vp, C.POINTER(AlignerParams), _vp, _vp, _vp, _vp, C.c_int32, _i32p, C.POINTER(AlignResult)]),
    "prs_pcf_linearize": (C.c_int, [_vp, C.POINTER(AlignerParams), _vp, _vp, C.c_int32, C.POINTER(AlignResult)]),
    "prs_gn_step": (C.c_int, [_vp, _vp, _vp, C.c_float, _vp]),
    "prs_gn_step_ex": (C.c_int, [_vp, _vp, _vp, C.c_float, C.c_int32, _vp]),
    "prs_selftest_reciprocal": (C.c_int, [_vp, _vp]),
    "prs_info_scale_from_nopt": (None, [_vp, C.c_int32, _vp]),
    "prs_triangulate": (C.c_int, [_vp, C.POINTER(TriangulatorParams), _vp, C.c_int32, _vp, _vp]),
    "prs_triangulate_dev": (C.c_int, [_vp, C.POINTER(TriangulatorParams), _vp, C.c_int64, _vp]),
    "prs_bruteforce_match_batch": (C.c_int, [_vp, C.POINTER(BruteforceParams), C.POINTER(BruteforceBatch)]),
    "prs_bruteforce_match": (C.c_int, [_vp, C.POINTER(BruteforceParams), _vp, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, _i32p]),
    "prs_extract_features_batch": (C.c_int, [_vp, C.POINTER(ExtractorParams), C.POINTER(ExtractBatch)]),
    "prs_selection_order": (C.c_int, [_vp, _vp, C.c_int32, _vp]),
    "prs_extract_features": (C.c_int, [_vp, C.POINTER(ExtractorParams), _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, _i32p]),
    "prs_extract_features_selective_batch": (C.c_int, [_vp, C.POINTER(SelectiveExtractorParams), C.POINTER(SelectiveExtractBatch)]),
    "prs_extract_features_selective": (C.c_int, [_vp, C.POINTER(SelectiveExtractorParams), _vp, C.c_int32, C.c_int32, C.c_int32, _vp,
                                                 C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_int32, _i32p]),
    "prs_depth_measurements_batch": (C.c_int, [_vp, C.POINTER(DepthParams), C.POINTER(DepthBatch)]),
    "prs_depth_measurements": (C.c_int, [_vp, C.POINTER(DepthParams), _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32,
                                         _vp, _vp, _vp, _i32p]),
    "prs_point_align_batch": (C.c_int, [_vp, C.POINTER(PointAlignParams), C.POINTER(PointAlignPairs)]),
    "prs_point_align": (C.c_int, [_vp, C.POINTER(PointAlignParams), _vp, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, _vp,
                                  C.POINTER(PointAlignResult), _vp]),
    "prs_place_db_create": (C.c_int, [_vp, C.POINTER(C.c_void_p)]),
    "prs_place_db_destroy": (C.c_int, [_vp]),
    "prs_place_db_clear": (C.c_int, [_vp]),
    "prs_place_db_reserve": (C.c_int, [_vp, C.c_int64, C.c_int64]),
    "prs_place_db_size": (C.c_int, [_vp, _i32p, _i32p, _i32p]),
    "prs_place_db_add": (C.c_int, [_vp, C.c_int64, _vp, _vp, _vp, C.c_int32]),
    "prs_place_query_batch": (C.c_int, [_vp, C.POINTER(PlaceParams), C.POINTER(PlaceQueries)]),
    "prs_place_query": (C.c_int, [_vp, C.POINTER(PlaceParams), C.c_int64, _vp, _vp, C.c_int32, _vp, _i32p, _vp, C.c_int32, _vp, _vp]),
    "prs_place_gather_pairs": (C.c_int, [_vp, C.POINTER(PlaceParams), C.POINTER(PlaceQueries), C.POINTER(PlacePairs)]),
    "prs_place_bank_create": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "prs_place_bank_destroy": (C.c_int, [_vp]),
    "prs_place_bank_clear": (C.c_int, [_vp]),
    "prs_place_bank_sizes": (C.c_int, [_vp, _vp, _vp, _vp]),
    "prs_place_bank_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_place_bank_bind_node_of_map": (C.c_int, [_vp, _vp]),
    "prs_place_bank_append_batch": (C.c_int, [_vp, C.POINTER(PlaceBankAppend)]),
    "prs_place_bank_query_batch": (C.c_int, [_vp, C.POINTER(PlaceParams), C.POINTER(PlaceQueries), C.POINTER(PlaceBankLinks)]),
    "prs_place_bank_gather_pairs": (C.c_int, [_vp, C.POINTER(PlaceParams), C.POINTER(PlaceQueries), C.POINTER(PlacePairs)]),
    "prs_pose_graph_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int64]),
    "prs_pose_graph_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_pose_graph_optimize_batch": (C.c_int, [_vp, C.POINTER(PoseGraphParams), C.POINTER(PoseGraphs)]),
    "prs_pose_graph_append_closures": (C.c_int, [_vp, C.POINTER(PoseGraphParams), C.POINTER(PoseGraphs), C.POINTER(PoseGraphClosures)]),
    "prs_pose_graph_optimize": (C.c_int, [_vp, C.POINTER(PoseGraphParams), C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp,
                                          C.POINTER(PoseGraphResult)]),
    "prs_pose_graph_lm_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int64]),
    "prs_pose_graph_lm_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_pose_graph_optimize_lm_batch": (C.c_int, [_vp, C.POINTER(PoseGraphLmParams), C.POINTER(PoseGraphs), _vp]),
    "prs_pose_graph_optimize_lm": (C.c_int, [_vp, C.POINTER(PoseGraphLmParams), C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp,
                                             C.POINTER(PoseGraphLmResult)]),
    "prs_pose_compose_batch": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp]),
    "prs_motion_predict_batch": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp]),
    "prs_merge_batch_run": (C.c_int, [_vp, C.POINTER(MergerParams), C.POINTER(MergeBatch)]),
    "prs_map_create": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    "prs_map_destroy": (C.c_int, [_vp]),
    "prs_map_clear": (C.c_int, [_vp]),
    "prs_map_reserve": (C.c_int, [_vp, C.c_int32]),
    "prs_map_size": (C.c_int, [_vp, _i32p, _i32p]),
    "prs_map_set_scene": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32]),
    "prs_map_set_frame_pose": (C.c_int, [_vp, C.c_int32, _vp]),
    "prs_map_merge": (C.c_int, [_vp, C.POINTER(MergerParams), _vp, _vp, _vp, _vp, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, _vp]),
    "prs_map_get_scene": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _i32p]),
    "prs_closure_merge_batch_run": (C.c_int, [_vp, C.POINTER(ClosureMergerParams), C.POINTER(ClosureMergeBatch)]),
    "prs_closure_merge_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_closure_merge": (C.c_int, [_vp, C.POINTER(ClosureMergerParams), C.c_int32, _i32p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    C.c_int32, _vp, C.c_int32, C.c_int32, _vp, C.c_int32, _vp]),
    "prs_map_merge_closure": (C.c_int, [_vp, C.POINTER(ClosureMergerParams), _vp, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp, C.c_int32,
                                        C.c_int32, _vp]),
    "prs_session_step_batch": (C.c_int, [_vp, C.POINTER(SessionParams), C.POINTER(SessionBatch)]),
    "prs_session_unroll_batch": (C.c_int, [_vp, C.POINTER(SessionBatch), _vp]),
    "prs_session_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_session_step_archive_batch": (C.c_int, [_vp, C.POINTER(SessionParams), C.POINTER(SessionBatch), C.POINTER(MergeBatch),
                                                 C.POINTER(MapArchive)]),
    "prs_session_reenter_batch": (C.c_int, [_vp, C.POINTER(ReentryParams), C.POINTER(SessionBatch), C.POINTER(MergeBatch),
                                            C.POINTER(MapArchive), C.POINTER(ReentryBatch)]),
    "prs_map_archive_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_context_get_dispatch_env": (C.c_int, [_vp, C.POINTER(DispatchEnv)]),
    "prs_stereo_plan": (C.c_int, [C.POINTER(StereoParams), C.POINTER(StereoBatch), C.POINTER(DispatchEnv), C.POINTER(DispatchPlan)]),
    "prs_align_plan": (C.c_int, [C.POINTER(PcfParams), C.POINTER(AlignerParams), C.POINTER(AlignBatch), C.c_int32, C.POINTER(DispatchEnv),
                                 C.POINTER(DispatchPlan)]),
    "prs_bruteforce_plan": (C.c_int, [C.POINTER(BruteforceParams), C.POINTER(BruteforceBatch), C.POINTER(DispatchEnv), C.POINTER(DispatchPlan)]),
    "prs_merge_plan": (C.c_int, [C.POINTER(MergerParams), C.POINTER(MergeBatch), C.POINTER(DispatchEnv), C.POINTER(DispatchPlan)]),
    "prs_dispatch_kernel_name": (C.c_char_p, [C.c_int32, C.c_int32]),
    "prs_dispatch_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_trajectory_eval_batch": (C.c_int, [_vp, C.POINTER(TrajectoryParams), C.POINTER(TrajectoryBatch)]),
    "prs_trajectory_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_world_map_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32]),
    "prs_world_map_batch_run": (C.c_int, [_vp, C.POINTER(WorldMapParams), C.POINTER(SessionBatch), C.POINTER(MergeBatch),
                                          C.POINTER(MapArchive), C.POINTER(WorldMapBatch)]),
    "prs_world_map_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_world_voxel_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32]),
    "prs_world_voxel_batch_run": (C.c_int, [_vp, C.POINTER(WorldVoxelParams), C.POINTER(WorldVoxelBatch)]),
    "prs_world_voxel_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_rectify_batch_run": (C.c_int, [_vp, C.POINTER(RectifyParams), C.POINTER(RectifyBatch)]),
    "prs_rectify_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_depth_cloud_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "prs_depth_cloud_batch_run": (C.c_int, [_vp, C.POINTER(DepthCloudParams), C.POINTER(DepthCloudBatch)]),
    "prs_depth_cloud_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_dense_stereo_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "prs_dense_stereo_batch_run": (C.c_int, [_vp, C.POINTER(DenseStereoParams), C.POINTER(DenseStereoBatch)]),
    "prs_dense_stereo_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_speckle_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "prs_speckle_batch_run": (C.c_int, [_vp, C.POINTER(SpeckleParams), C.POINTER(SpeckleBatch)]),
    "prs_speckle_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_sgm_stereo_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "prs_sgm_stereo_batch_run": (C.c_int, [_vp, C.POINTER(SgmStereoParams), C.POINTER(SgmStereoBatch)]),
    "prs_sgm_stereo_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_depth_consistency_workspace_bytes": (C.c_uint64, [C.c_int32, C.c_int32, C.c_int32]),
    "prs_depth_consistency_batch_run": (C.c_int, [_vp, C.POINTER(DepthConsistencyParams), C.POINTER(DepthConsistencyBatch)]),
    "prs_depth_consistency_struct_sizes": (None, [C.POINTER(C.c_uint64)]),
    "prs_scene_clip_batch": (C.c_int, [_vp, C.POINTER(Projector), _vp, C.POINTER(ClipBatch)]),
    "prs_scene_clip": (C.c_int, [_vp, C.POINTER(Projector), _vp, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, C.c_int32, _i32p]),
}

# every *_struct_sizes entry with the mirrors of the structs it reports, in the order its function writes them; load() compares them
STRUCT_SIZES = (
    ("prs_guard_struct_sizes", (GuardExtent, GuardRegion)),
    ("prs_place_bank_struct_sizes", (PlaceBankAppend, PlaceBankLinks)),
    ("prs_pose_graph_struct_sizes", (PoseGraphParams, PoseGraphResult, PoseGraphs, PoseGraphClosures)),
    ("prs_pose_graph_lm_struct_sizes", (PoseGraphLmParams, PoseGraphLmResult)),
    ("prs_closure_merge_struct_sizes", (ClosureMergerParams, ClosureMergeBatch)),
    ("prs_session_struct_sizes", (SessionParams, SessionBatch)),
    ("prs_map_archive_struct_sizes", (MapArchive, ReentryParams, ReentryBatch)),
    ("prs_dispatch_struct_sizes", (DispatchEnv, DispatchPlan)),
    ("prs_trajectory_struct_sizes", (TrajectoryParams, TrajectoryResult, TrajectoryBatch)),
    ("prs_world_map_struct_sizes", (WorldMapParams, WorldMapBatch)),
    ("prs_world_voxel_struct_sizes", (WorldVoxelParams, WorldVoxelBatch)),
    ("prs_rectify_struct_sizes", (RectifyMap, RectifyParams, RectifyBatch)),
    ("prs_depth_cloud_struct_sizes", (DepthCloudParams, DepthCloudBatch)),
    ("prs_dense_stereo_struct_sizes", (DenseStereoParams, DenseStereoBatch)),
    ("prs_speckle_struct_sizes", (SpeckleParams, SpeckleBatch)),
    ("prs_sgm_stereo_struct_sizes", (SgmStereoParams, SgmStereoBatch)),
    ("prs_depth_consistency_struct_sizes", (DepthConsistencyParams, DepthConsistencyBatch)),
)


def c_name(mirror):
    """the header struct a mirror stands for: the first word of its docstring"""
    return mirror.__doc__.split()[0].rstrip(":")


_lib = None


class ProslamHipError(RuntimeError):
    """hard error from the C-ABI (status < 0); the reference throws std::runtime_error here"""

    def __init__(self, status, message):
        super().__init__("libproslam_hip status %d: %s" % (status, message))
        self.status = status


def load():
    """dlopen the product library and bind every declared symbol; raises if it is absent"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libproslam_hip.so is not built (%s). The HIP extension is mandatory: run "
            "`python -c 'import __graft_entry__ as g; g.build()'` -- there is no CPU fallback." % LIB_PATH)
    # torch bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Import it FIRST so the
    # dynamic loader resolves our DT_NEEDED against the runtime torch already mapped: one HIP
    # runtime per process, so torch tensors / streams and this library agree.  Two runtime
    # copies in one process fail HSA initialisation for the second one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    # the ctypes mirrors above and the library must describe the same structs (include/proslam_hip.h, PRS_ABI_VERSION)
    rc = lib.prs_abi_check(ABI_VERSION, C.sizeof(StereoParams), C.sizeof(PcfParams), C.sizeof(AlignerParams), C.sizeof(AlignBatch))
    if rc != 0:
        raise ImportError("libproslam_hip.so (version %d) does not match the Python binding (version %d, struct sizes %d/%d/%d/%d): "
                          "rebuild with `python -c 'import __graft_entry__ as g; g.build()'`"
                          % (lib.prs_version(), ABI_VERSION, C.sizeof(StereoParams), C.sizeof(PcfParams), C.sizeof(AlignerParams), C.sizeof(AlignBatch)))
    # the structs of the later sections have their own size queries
    for query, mirrors in STRUCT_SIZES:
        sizes = (C.c_uint64 * len(mirrors))()
        getattr(lib, query)(sizes)
        mine = [C.sizeof(m) for m in mirrors]
        if list(sizes) != mine:
            raise ImportError("libproslam_hip.so lays out %s as %s bytes, the Python binding as %s: rebuild with "
                              "`python -c 'import __graft_entry__ as g; g.build()'`"
                              % (" / ".join(c_name(m) for m in mirrors), list(sizes), mine))
    _lib = lib
    return lib
