/*
 * proslam_hip.h -- C-ABI of libproslam_hip.so: the MI355X (gfx950) implementation of
 * srrg2_proslam's per-frame tracking hot path.
 *
 * Every entry point names the reference interface it replaces (paths relative to
 * /root/reference/srrg2_proslam/src/srrg2_proslam/; CF/ = registration/correspondence_finders/).
 * The boundary is plain C: pointers, sizes, POD structs.  No torch / Eigen / OpenCV types.
 *
 * Two flavours of every operator:
 *   - "host" calls take host pointers for ONE frame and are what a srrg2 plugin adapter's
 *     compute() binds; they upload, launch, download and synchronise.
 *   - "_batch" calls take DEVICE pointers for B independent frames (one per sequence), enqueue
 *     on the context's HIP stream and return without synchronising.  Per-frame status words are
 *     written to device memory.
 *
 * Status convention (mirrors the reference's error behaviour):
 *   0      ok
 *   < 0    hard error (the reference throws std::runtime_error: CF/..bruteforce_impl.cpp:203-216)
 *   > 0    OR of warning bits (the reference prints a warning and returns:
 *          CF/..bruteforce_impl.cpp:217-226,237-242; CF/..epipolar_impl.cpp:211-216;
 *          CF/..projective_base_impl.cpp:228-263)
 *
 * Supported domain of the device kernels (checked; violations are hard errors, never silent):
 *   keypoint coordinates 0 <= u < 32768, 0 <= v < image_rows <= 4096; keypoints per image <= 8192
 *   (stereo matcher) / fixed points <= 32767 (lattice finder, the reference's own int16 limit,
 *   CF/correspondence_finder_projective_square_impl.cpp:20-22).
 *
 * Extent of a device array (what the caller must own; tests/test_guard_*_gpu.py run the entry points they cover with nothing more):
 *   - an array [batch][stride][...] has batch * stride whole rows, also where a count is below its stride; rows from the count to
 *     the stride are neither read nor written unless the entry point says so;
 *   - a pitched image array [images][rows][pitch] ends at the LAST PIXEL of the last row of the last image:
 *     ((images * rows - 1) * pitch + cols * element size) bytes.  The padding behind the last row need not exist, so a view of the
 *     right half of a side-by-side allocation, whose last row ends where the allocation ends, is a valid argument.  Padding between
 *     rows is never written and its values reach no result.  This holds for images and seeding_mask of the two extractors, depth of
 *     prs_depth_batch, dst of the rectifier, depth and gray of the dense cloud, left, right, disparity and depth of both stereo
 *     stages, image, companion and label of the speckle filter and depth, out, support and violation of the consistency filter.
 *     The one exception is src of prs_rectify_batch when src and src_pitch are both multiples of 16 bytes (see there): its last row
 *     then has cols * element size rounded up to 16 bytes, which lies inside the pitch;
 *   - a workspace has exactly the bytes its prs_*_workspace_bytes function returns for the sizes and switches of that call; it need
 *     not be cleared.
 */
#ifndef PROSLAM_HIP_H
#define PROSLAM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRS_API __attribute__((visibility("default")))
#define PRS_DESC_BYTES 32 /* 256-bit binary descriptor row (cv::Mat 1x32 CV_8U in the reference) */

/* ---- status ---- */
enum {
  PRS_OK                 = 0,
  PRS_WARN_EMPTY_INPUT   = 1,  /* CF/..bruteforce_impl.cpp:217-226 */
  PRS_WARN_NO_MATCHES    = 2,  /* CF/..bruteforce_impl.cpp:237-242 */
  PRS_WARN_LOW_RATIO     = 4,  /* CF/..epipolar_impl.cpp:211-216, CF/..projective_base_impl.cpp:228-232 */
  PRS_WARN_RETRIED       = 8,  /* CF/..projective_base_impl.cpp:235-249 */
  PRS_WARN_TRACK_LOST    = 16, /* CF/..projective_base_impl.cpp:251-259 */
  PRS_WARN_NO_PROJECTION = 32, /* CF/..projective_base_impl.cpp:167-171 */
  PRS_ERR_NULL           = -1, /* unset input (reference: throw) */
  PRS_ERR_CAPACITY       = -2, /* output buffer too small */
  PRS_ERR_HIP            = -3, /* HIP runtime failure; see prs_last_error() */
  PRS_ERR_RANGE          = -4, /* input outside the supported domain (see above) */
  PRS_ERR_UNSUPPORTED    = -5, /* size beyond kernel limits */
  PRS_ERR_NO_DEVICE      = -6  /* no MI355X-class device visible */
};

/* Correspondence{int fixed_idx, int moving_idx, float response}
 * (srrg2_core, emitted at CF/..epipolar_impl.cpp:177-178) */
typedef struct {
  int32_t fixed_idx;
  int32_t moving_idx;
  float response;
} prs_corr;

/* image-plane keypoint (coordinates()(0), coordinates()(1)) */
typedef struct {
  float u;
  float v;
} prs_kp2;

/* ---- context: one device, one stream, scratch memory.  Not re-entrant (the reference's
 *      finders are not either); different contexts are independent. ---- */
typedef struct prs_context prs_context;
PRS_API int prs_context_create(int device_id, prs_context** ctx);
PRS_API int prs_context_destroy(prs_context* ctx);
/* enqueue on a caller-owned hipStream_t (e.g. torch's current stream); NULL = HIP's default stream */
PRS_API int prs_context_set_stream(prs_context* ctx, void* hip_stream);
/* go back to the non-blocking stream the context created for itself (the initial state) */
PRS_API int prs_context_use_own_stream(prs_context* ctx);
PRS_API int prs_context_synchronize(prs_context* ctx);
/* measurement: when on, prs_align_batch_run brackets every launch of its two kernels (projective search, Gauss-Newton
 * rounds) with HIP events on the context's stream and accumulates their durations; enabling resets the sums */
PRS_API int prs_context_enable_timing(prs_context* ctx, int32_t on);
PRS_API int prs_context_get_align_timing(prs_context* ctx, double* search_ms, double* gn_ms, int64_t* search_launches, int64_t* gn_launches);
/* the same sums by round of the batch: search_ms16[r] / gn_ms16[r] = total time of the r-th search / Gauss-Newton launch over
 * `batches` timed batches (round 15 collects every later round) */
PRS_API int prs_context_get_align_round_timing(prs_context* ctx, double* search_ms16, double* gn_ms16, int64_t* batches);
/* diagnostic, for tests and profiles: which path the later projective searches of the context's LAST FINISHED aligner batch
 * took (a batch that ran the fused kernel reports 0 / 0, whatever a split batch before it counted). A later search of a frame loop settles a query from the frame's query cache (a hit: its cell rectangle lies inside the
 * one its last pruned scan covered) or scans it again (a miss); both are summed over the batch's frames and later searches.  0 / 0
 * when no search read the cache: PRS_NO_SEARCH_REUSE=1, the KD-tree finder, eight survivor slots, unpruned searches, the fused
 * kernel.  One device-to-host copy of the frame control words and a stream synchronise; PRS_ERR_UNSUPPORTED while a batch is
 * enqueued and not finished.  Results never depend on the path. */
PRS_API int prs_context_get_search_reuse(prs_context* ctx, int64_t* hits, int64_t* misses);
/* Dense phase of the brute-force matcher (prs_bruteforce_match_batch): which kernels score the N_f x N_m pairs.  Results are
 * identical; only the cost differs.
 *   PRS_BF_DENSE_MATRIX_WHEN_FULL (the default): a batch of 32 or more cloud pairs (of at least 256 x 64 points) runs one workgroup
 *     per pair with the distances from v_mfma_i32_16x16x64_i8 (exact: integer products) and the registration state in LDS; fewer pairs
 *     run the popcount kernels, which spread a pair over several workgroups.  On real cloud pairs (KITTI stereo pairs, ~750 points a
 *     side, 1.6 % of the pairs within 50 bits) 1.8x the popcount kernels at 1024 pairs and 2x at 128, on 1024 pairs of uniform random
 *     rows 2.7x; 32 - 63 pairs of uniform random rows are the one shape it loses on (0.23 against 0.14 ms) (profiles/r06/README.md).
 *   PRS_BF_DENSE_POPCOUNT: v_xor / v_bcnt on the vector units for every batch size.
 *   PRS_BF_DENSE_MATRIX: always the matrix cores (the fused shape where it applies, else a split matrix-core kernel + a registration
 *     launch that re-scores what it selects: fast on uniform random rows, slow on real ones; tests, A-B runs).
 * The environment variable PRS_BF_MFMA (0 / auto / 1), read when the context is created, sets the initial mode. */
#define PRS_BF_DENSE_POPCOUNT 0
#define PRS_BF_DENSE_MATRIX_WHEN_FULL 1
#define PRS_BF_DENSE_MATRIX 2
PRS_API int prs_context_set_bruteforce_dense_phase(prs_context* ctx, int32_t mode);
PRS_API const char* prs_last_error(const prs_context* ctx);
PRS_API const char* prs_status_string(int status);
PRS_API int prs_version(void);
/* The launch-size rule every entry point applies to every launch of a call before the first one: HIP takes no launch of 2^32 or more work-items in a grid
 * dimension, so a launch of `workgroups` workgroups of `threads` threads fits iff workgroups >= 1, 1 <= threads <= 1024 and
 * workgroups * threads <= 2^32 - 1 -- 2^24 - 1 workgroups of 256 threads.  1 when it fits, else 0 (pure: no context, no device). */
PRS_API int prs_launch_fits(int64_t workgroups, int32_t threads);
/* ---- guard mode: the library's own device and pinned memory between guard bands (tests and tools).
 * Every block the library allocates -- the context's work, staging and pinned arenas, the aligner's six job buffers, the arrays of a
 * prs_map, a prs_pcf handle's device and pinned block, a place database's and a place bank's arrays, the information table -- goes
 * through one allocation path, each with a short name.  The environment variable PRS_GUARD_FILL=00 or ff, read when the context is
 * created (any other value: off), turns guard mode on for that context and everything created on it:
 *   - a block is [front band | user bytes | tail band].  The front band has PRS_GUARD_BAND bytes, so the user pointer keeps the
 *     allocator's alignment; the tail band begins at the first byte behind the bytes the site requested, without rounding, and has
 *     max(PRS_GUARD_BAND, the slack the site's rule adds to that request with guard off) bytes: whatever stays inside its block
 *     without guard mode stays inside it with it, so guard mode cannot turn a silent overrun into a fault.  Both bands are painted
 *     with PRS_GUARD_PATTERN, the user bytes with the fill;
 *   - the grow-only blocks whose contents belong to whatever call runs next -- every work and staging arena, the pinned arena, the
 *     aligner's job buffers -- are painted with the fill again at every request, on the stream in front of the launches.  Memory that
 *     carries state between calls (a prs_map, a prs_pcf handle's block, a place database or bank, the information table) is painted
 *     when it is allocated only;
 *   - before a block is freed -- by growth, by a handle's destroy, by prs_context_destroy -- its bands are checked, and a damaged
 *     one is latched in the context with its name.  prs_context_destroy prints what is latched to stderr and returns the count.
 * With guard mode off every site requests the bytes it always did (prs_guard_layout with guard = 0 is that rule) and nothing is
 * painted or checked.
 * prs_guard_layout: the layout rule (pure: no context, no device).  slack_rule: PRS_GUARD_SLACK_EXACT (bytes), _QUARTER
 * (bytes + bytes / 4 + 4096: the work arenas, the small staging arenas, the aligner's job buffers) or _HALF (bytes + bytes / 2 + 4096:
 * the default staging arena and the pinned arena).  With guard = 0: total = that size, user_offset = 0, tail_bytes = the slack.
 * PRS_ERR_NULL without `out`, PRS_ERR_UNSUPPORTED for an unknown rule.
 * prs_context_guard_regions: the context's live blocks in allocation order, at most `capacity` of them written; returns how many
 * there are.  prs_context_guard_check: synchronises the context's stream, copies every live block's bands to the host and returns
 * the number of damaged (block, side) pairs, those latched from freed blocks included; `report` (may be NULL) receives one line
 * "name front|tail offset" for each, offset = the first damaged byte counted from the band's start, truncated to report_bytes with
 * a terminating 0.  Both return PRS_ERR_UNSUPPORTED on a context that is not in guard mode. */
#define PRS_GUARD_SLACK_EXACT 0
#define PRS_GUARD_SLACK_QUARTER 1
#define PRS_GUARD_SLACK_HALF 2
#define PRS_GUARD_BAND 4096
#define PRS_GUARD_PATTERN 0xA5
typedef struct {
  uint64_t total;       /* bytes the allocator is asked for */
  uint64_t user_offset; /* of the user bytes in the block */
  uint64_t tail_bytes;  /* behind the user bytes: the tail band, or with guard off the slack */
} prs_guard_extent;
typedef struct {
  void* user;          /* first user byte (device memory, or pinned host memory) */
  uint64_t bytes;      /* user bytes: what the site requested when it allocated the block */
  uint64_t tail_bytes; /* the tail band, at user + bytes */
  int32_t pinned;      /* 1: pinned host memory */
  int32_t reserved;
  char name[48];
} prs_guard_region;
PRS_API int prs_guard_layout(uint64_t bytes, int32_t slack_rule, int32_t guard, prs_guard_extent* out);
PRS_API int prs_context_guard_check(prs_context* ctx, char* report, uint64_t report_bytes);
PRS_API int prs_context_guard_regions(prs_context* ctx, prs_guard_region* out, int32_t capacity);
PRS_API void prs_guard_struct_sizes(uint64_t* sizes2);
/* The parameter structs below carry no size field and grow at their END between versions (round 5 added three int32 fields to
 * prs_aligner_params).  PRS_ABI_VERSION is what this header describes, prs_version() what the loaded library was built from; a
 * client checks that they agree once (prs_abi_check: also the sizes of the structs it will pass, as the client's compiler laid
 * them out) instead of finding out through a library that reads past a shorter struct (101 -> 102: step_norm_exit at the end of
 * prs_aligner_params; 102 also adds the entry points prs_abi_check and prs_context_set_bruteforce_dense_phase; 103 adds the
 * selective extractor: prs_selective_extractor_params, prs_selective_extract_batch and their two entry points, no existing struct changed; 104 adds
 * the RGB-D preprocessor: prs_depth_params, prs_depth_batch and their two entry points, no existing struct changed; the loop aligner's
 * prs_point_align_params, prs_point_align_pairs, prs_point_align_result and its two entry points came later under the same version:
 * new structs and new entry points only, nothing a 104 client passes changed; so did the loop detector's place database:
 * prs_place_db, prs_place_params, prs_place_queries, prs_place_pairs and the prs_place_* entry points; and the pose-graph optimiser:
 * prs_pose_graph_params, prs_pose_graph_result, prs_pose_graphs, prs_pose_graph_closures, the prs_pose_graph_* entry points and the
 * status PRS_ERR_NOT_POSITIVE_DEFINITE; and its Levenberg-Marquardt form: prs_pose_graph_lm_params, prs_pose_graph_lm_result and the
 * prs_pose_graph_lm_* / prs_pose_graph_optimize_lm* entry points; and the closure merger: prs_closure_merger_params,
 * prs_closure_merge_batch, the prs_closure_merge* entry points and prs_map_merge_closure; and the local-map manager:
 * prs_session_params, prs_session_batch and the prs_session_* entry points; and the place bank: prs_place_bank,
 * prs_place_bank_append, prs_place_bank_links and the prs_place_bank_* entry points; and map re-entry: prs_map_archive,
 * prs_reentry_params, prs_reentry_batch, prs_session_step_archive_batch, prs_session_reenter_batch and
 * prs_map_archive_struct_sizes; and the dispatch plans for tests and tools: prs_dispatch_env,
 * prs_dispatch_plan, prs_context_get_dispatch_env, the prs_*_plan entry points, prs_dispatch_kernel_name and
 * prs_dispatch_struct_sizes; and the trajectory evaluator: prs_trajectory_params, prs_trajectory_result, prs_trajectory_batch,
 * prs_trajectory_eval_batch and prs_trajectory_struct_sizes; and the search's query-cache read-out prs_context_get_search_reuse
 * with prs_dispatch_env::no_search_reuse at the end of that tests-and-tools struct; and the world map: prs_world_map_params,
 * prs_world_map_batch, prs_world_map_workspace_bytes, prs_world_map_batch_run and prs_world_map_struct_sizes; and the world voxel filter:
 * prs_world_voxel_params, prs_world_voxel_batch, prs_world_voxel_workspace_bytes, prs_world_voxel_batch_run and
 * prs_world_voxel_struct_sizes; and the image rectifier: prs_rectify_map, prs_rectify_params, prs_rectify_batch, prs_rectify_batch_run
 * and prs_rectify_struct_sizes; and the dense RGB-D cloud: prs_depth_cloud_params, prs_depth_cloud_batch,
 * prs_depth_cloud_workspace_bytes, prs_depth_cloud_batch_run and prs_depth_cloud_struct_sizes; and dense stereo:
 * prs_dense_stereo_params, prs_dense_stereo_batch, prs_dense_stereo_workspace_bytes, prs_dense_stereo_batch_run and
 * prs_dense_stereo_struct_sizes; and the speckle filter: prs_speckle_params, prs_speckle_batch, prs_speckle_workspace_bytes,
 * prs_speckle_batch_run and prs_speckle_struct_sizes; and semi-global dense stereo: prs_sgm_stereo_params, prs_sgm_stereo_batch,
 * prs_sgm_stereo_workspace_bytes, prs_sgm_stereo_batch_run and prs_sgm_stereo_struct_sizes; and the depth consistency filter:
 * prs_depth_consistency_params, prs_depth_consistency_batch, prs_depth_consistency_workspace_bytes, prs_depth_consistency_batch_run
 * and prs_depth_consistency_struct_sizes; and guard mode for tests and tools: prs_guard_extent, prs_guard_region, prs_guard_layout,
 * prs_context_guard_check, prs_context_guard_regions and prs_guard_struct_sizes).  Callers memset() parameter structs before
 * filling them, so that fields they do not know select the shipped defaults (all zero). */
#define PRS_ABI_VERSION 104
PRS_API int prs_abi_check(int32_t header_version, uint64_t sizeof_stereo_params, uint64_t sizeof_pcf_params, uint64_t sizeof_aligner_params,
                          uint64_t sizeof_align_batch);
#define PRS_ABI_CHECK() prs_abi_check(PRS_ABI_VERSION, sizeof(prs_stereo_params), sizeof(prs_pcf_params), sizeof(prs_aligner_params), sizeof(prs_align_batch))

/* ================================================================================================
 * Stereo epipolar matcher
 * replaces CorrespondenceFinderDescriptorBasedEpipolar<..>::compute (CF/..epipolar_impl.cpp:46-219)
 * incl. Feature/_sortFeatureVector (:8-42) and the pre/post contract (CF/..bruteforce_impl.cpp:203-243)
 * ============================================================================================== */
typedef struct {
  float maximum_descriptor_distance;           /* CF/..bruteforce.h:22-26 */
  float maximum_distance_ratio_to_second_best; /* CF/..bruteforce.h:27-31 */
  float minimum_matching_ratio;                /* CF/..bruteforce.h:32-36 */
  int32_t maximum_disparity_pixels;            /* CF/..epipolar.h:22-26 */
  int32_t epipolar_line_thickness_pixels;      /* CF/..epipolar.h:28-32 */
  int32_t image_rows;                          /* extent of the row table: 0 <= v < image_rows */
  int32_t image_cols;                          /* reserved (the column-binned kernel of round 1 was removed); ignored */
} prs_stereo_params;

/* triangulation parameters, TriangulatorRigidStereo (mapping/triangulator_rigid_stereo.h:34-58,
 * .cpp:88-109): b_x = (K * t_right_in_left).x */
typedef struct {
  float fx, fy, cx, cy;
  float b_x;
  float minimum_disparity_pixels;
  float infinity_depth_meters;
} prs_triangulator_params;

/* host, one frame.  fixed = left keypoints, moving = right keypoints
 * (sensor_processing/raw_data_preprocessor_stereo_projective.cpp:99-102).
 * out: capacity >= n_left; order = sorted-left traversal per offset pass like the reference. */
PRS_API int prs_stereo_match(prs_context* ctx,
                             const prs_stereo_params* params,
                             const prs_kp2* left,
                             const uint8_t* desc_left,
                             int32_t n_left,
                             const prs_kp2* right,
                             const uint8_t* desc_right,
                             int32_t n_right,
                             prs_corr* out,
                             int32_t capacity,
                             int32_t* n_out);

/* device-resident batch: frame b uses element range [b*stride, b*stride + n[b]) of every array.
 * Optional fused "adaptor + triangulator" epilogue (all four pointers non-NULL to enable):
 * replaces the assembly loop of RawDataPreprocessorStereoProjective::compute
 * (sensor_processing/raw_data_preprocessor_stereo_projective.cpp:107-132: (uL,vL,uR,vR) points,
 * matches with negative horizontal or vertical disparity dropped, left descriptor kept) and
 * TriangulatorRigidStereo::compute (mapping/triangulator_rigid_stereo.cpp:7-56) on its output. */
typedef struct {
  int32_t batch;
  int32_t stride;            /* keypoint capacity per image and frame (elements) */
  const prs_kp2* left_kp;    /* [batch][stride], 8-byte aligned (so is right_kp) */
  const uint8_t* left_desc;  /* [batch][stride][32], 16-byte aligned (so are right_desc and the epilogue's fixed_uvuv, fixed_desc, fixed_xyz) */
  const int32_t* n_left;     /* [batch] */
  const prs_kp2* right_kp;
  const uint8_t* right_desc;
  const int32_t* n_right;
  prs_corr* matches;         /* [batch][stride] */
  int32_t* n_matches;        /* [batch] */
  int32_t* status;           /* [batch] */
  /* optional epilogue outputs (NULL to skip) */
  float* fixed_uvuv;         /* [batch][stride][4]  (uL,vL,uR,vR) */
  uint8_t* fixed_desc;       /* [batch][stride][32] left descriptor of the match */
  int32_t* n_fixed;          /* [batch] */
  float* fixed_xyz;          /* [batch][stride][4]  triangulated (x,y,z, valid ? 1 : 0) */
  const prs_triangulator_params* triangulator; /* HOST pointer, read at enqueue */
} prs_stereo_batch;

/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): the unstaged kernel of frames beyond 2048 keypoints has a workgroup of 1024 threads a frame, batch <= 2^22 - 1;
 * the staged kernels launch no more workgroups than the device has compute units. */
PRS_API int prs_stereo_match_batch(prs_context* ctx,
                                   const prs_stereo_params* params,
                                   const prs_stereo_batch* batch);

/* ================================================================================================
 * Rectified stereo triangulation
 * replaces TriangulatorRigidStereo::compute / triangulateRectifiedMidpoint
 * (mapping/triangulator_rigid_stereo.cpp:7-56,60-85).  Output size == input size; points with
 * uL - uR < minimum_disparity_pixels are flagged invalid (valid[i] = 0, xyz = 0).
 * ============================================================================================== */
PRS_API int prs_triangulate(prs_context* ctx,
                            const prs_triangulator_params* params,
                            const float* uvuv, /* host [n][4] */
                            int32_t n,
                            float* xyz,        /* host [n][3] */
                            uint8_t* valid);   /* host [n] */

/* device: uvuv [n][4] -> xyz4 [n][4] = (x, y, z, valid), both 16-byte aligned (a row moves as one float4; PRS_ERR_UNSUPPORTED
 * otherwise, nothing launched).  At most 2048 workgroups stride over the points: any n fits one launch */
PRS_API int prs_triangulate_dev(prs_context* ctx,
                                const prs_triangulator_params* params,
                                const float* d_uvuv,
                                int64_t n,
                                float* d_xyz4);

/* ================================================================================================
 * Projective correspondence finder + reprojection-error Gauss-Newton aligner
 * replaces CorrespondenceFinderProjectiveBase<..>::compute and its Square / Circle / Rhombus /
 * KDTree search patterns (CF/correspondence_finder_projective_base_impl.cpp:105-293,
 * CF/..square_impl.cpp:8-118, CF/..circle_impl.cpp:8-94, CF/..rhombus_impl.cpp:8-93,
 * CF/..kdtree_impl.cpp:8-80), AlignerSliceProcessorProjective{,Depth,Stereo}::setupFactor
 * (registration/aligner_slice_processor_projective.cpp:28-112) and the external arithmetic those
 * configure (srrg2_solver SE3*ProjectiveErrorFactor::errorAndJacobian, RobustifierSaturated,
 * H/b accumulation, damped GN step, MultiAligner3DQR iteration loop).
 * ============================================================================================== */
/* PRS_SEARCH_KDTREE = CorrespondenceFinderProjectiveKDTree (CF/..projective_kdtree_impl.cpp:8-80) over srrg2_core::KDTree<float, 2>
 * (external), restated from its published construction with the constants the reference's own pinned results fix: a cluster
 * is split at its mean along the direction of largest variance until it holds fewer than minimum_number_of_points_per_cluster
 * points or 3 * sqrt(largest eigenvalue of its covariance) < leaf range (= the search radius when _initializeDatabase ran,
 * kept in prs_pcf_state.database_leaf_range); findNeighbors(query, r^2) returns the members of the ONE leaf the query descends
 * to that lie within r.  This reproduces the eight counts the reference asserts for the finder (319, 2, 120, 21, 82, 36, 104, 56:
 * tests/test_correspondence_finders.cpp:330-609); an exhaustive radius search would return supersets.
 * Arithmetic (BUILD-DEFINED): cluster sums as exact integers of the coordinates in 1/16 px, mean / covariance / eigenvector in
 * double, node = (mean, unit normal) in float, side (x - mean_x) * n_x + (y - mean_y) * n_y < 0 -> left in float, leaf members in
 * ascending fixed index; |u|, |v| < 32768.  Clusters beyond the LDS carve of max_fixed (about max_fixed / 3 inner nodes) give
 * PRS_ERR_CAPACITY for that frame. */
enum { PRS_SEARCH_KDTREE = 0, PRS_SEARCH_SQUARE = 1, PRS_SEARCH_CIRCLE = 2, PRS_SEARCH_RHOMBUS = 3 };
enum { PRS_FACTOR_MONO = 2, PRS_FACTOR_DEPTH = 3, PRS_FACTOR_STEREO = 4 }; /* = fixed dimension */

/* PointProjectorPinhole_ parameters reached through param_projector (CF/..projective_base.h:55-59) */
typedef struct {
  float fx, fy, cx, cy;
  int32_t canvas_cols, canvas_rows;
  float range_min, range_max;
} prs_projector;

typedef struct {
  float maximum_descriptor_distance;           /* CF/..bruteforce.h:22-26 */
  float maximum_distance_ratio_to_second_best; /* CF/..bruteforce.h:27-31 */
  float minimum_matching_ratio;                /* CF/..bruteforce.h:32-36 */
  float minimum_descriptor_distance;           /* CF/..projective_base.h:30-34 */
  float descriptor_distance_step_size_pixels;  /* :35-39 */
  uint64_t maximum_search_radius_pixels;       /* :40-44 */
  uint64_t minimum_search_radius_pixels;       /* :45-49 */
  uint64_t search_radius_step_size_pixels;     /* :50-54 */
  uint64_t minimum_number_of_iterations;       /* :60-64 */
  float maximum_estimate_change_norm_for_convergence; /* :65-69 */
  uint64_t number_of_solver_iterations_per_projection; /* :70-74 */
  int32_t search_type;                         /* which subclass: PRS_SEARCH_* */
  prs_projector projector;
  int32_t minimum_number_of_points_per_cluster; /* KD-tree finder only (CF/..projective_kdtree.h:24-28); 0 = its default, 10 */
} prs_pcf_params;

/* the finder members that live across calls and frames (CF/..projective_base.h:132-154).  POD so
 * it can sit in device memory for the batched path; zero-initialise, then set config_changed = 1. */
typedef struct {
  uint64_t search_radius_pixels;
  uint64_t current_iteration;
  float descriptor_distance;
  int32_t has_converged;
  int32_t config_changed;
  int32_t num_recomputes; /* bookkeeping only: number of full searches so far */
  float local_map_in_sensor[16];
  float local_map_in_sensor_previous[16];
  float database_leaf_range; /* KD-tree finder: _search_radius_pixels when _initializeDatabase last ran (the tree's leaf range) */
  int32_t reserved; /* internal hint, no result depends on it: bit 0 = the search has stopped pruning candidates by partial descriptor
                       distances for this finder (its rows are correlated: more than an eighth of a search's queries overflowed) */
} prs_pcf_state;

typedef struct {
  int32_t factor_type;                    /* PRS_FACTOR_*: which error factor / fixed dimension */
  float fx, fy, cx, cy;                   /* factor->setCameraMatrix (aligner_slice_processor_projective.cpp:36-37) */
  float image_cols, image_rows;           /* factor->setImageDim (:38-39) */
  float baseline_left_in_right_px[3];     /* K * t_left_in_right (:98-104), stereo only */
  float diagonal_info[3];                 /* param_diagonal_info_matrix (:47) */
  float chi_threshold;                    /* RobustifierSaturated chi_threshold: a factor with chi > threshold is kernelised,
                                             its Omega scaled by 1 / chi, its chi reported as the threshold (*) */
  int32_t enable_inverse_depth_weighting; /* :107-112: translation columns of J scaled by min(0.01 + d / mean disparity, 1) (*) */
  float mean_disparity;                   /* bindFixed (:76-89); < 0 = compute it on the device */
  float damping;                          /* IterationAlgorithmGN damping: (H + damping diag(H)) dx = -b (*)
                                             (*) srrg2_solver is not in the reference tree; these three readings are the family under
                                             which every pose bound of the reference's gtests holds */
  int32_t max_iterations;                 /* MultiAligner3DQR max_iterations */
  int32_t min_num_inliers;
  int32_t min_num_correspondences;
  int32_t stop_at_fixed_point;            /* 1: leave the loop once the finder has converged and a GN
                                             step reproduces the estimate bit-for-bit (every remaining
                                             iteration would repeat it exactly); 0: always run all */
  /* MultiAligner3DQR flags of the RGB-D configurations (configurations/icl.conf:50-64, tum.conf:90-104; both 0 in
   * kitti.conf:980-1010 / euroc.conf).  The class is external and its loop is not pinned by anything in the reference
   * tree, so the semantics are BUILD-DEFINED:
   *   enable_inlier_only_runs ("toggles additional inlier only runs if sufficient inliers are available"): after the
   *     max_iterations loop, if the last linearisation had >= min_num_inliers inliers, inlier_only_iterations
   *     (<= 0: max_iterations) further Gauss-Newton iterations on the frozen correspondence vector (the finder is not
   *     called) in which kernelised factors (chi2 > threshold) are suppressed instead of saturated;
   *   keep_only_inlier_correspondences ("toggles removal of correspondences which factors are not inliers in the last
   *     iteration"): the returned vector keeps the inliers of the last linearisation, order preserved. */
  int32_t enable_inlier_only_runs;
  int32_t keep_only_inlier_correspondences;
  int32_t inlier_only_iterations;
  /* AlignerSliceProcessorProjective{,Depth,Stereo}WithSensor (aligner_slice_processor_projective.h:80-83,88-91,
   * tests/test_aligners.cpp:142-584): the estimate X is the ROBOT's movingInFixed; points reach the camera through
   * A = sensor_in_robot^-1 * X, which is what the finder projects with and the factor linearises at; the
   * perturbation stays on X.  sensor_in_robot: row-major 4x4 (Platform::getTransform(frame_id, base_frame_id)). */
  int32_t with_sensor;
  float sensor_in_robot[16];
  /* AlignerSliceMotionModel3D + MotionModelConstantVelocity3D (configurations/kitti.conf:257-260,747-772; external,
   * the .conf gives the slice no information matrix: identity assumed, BUILD-DEFINED): prior factor
   * e = t2tnq(Z^-1 X), J = I, H += diag(motion_prior_info), b += motion_prior_info * e, re-evaluated every iteration.
   * Z = prs_align_batch.prior_mean (NULL = identity: the local map was clipped at the motion-model prediction). */
  int32_t enable_motion_prior;
  float motion_prior_info[6];
  /* Readings of the un-vendored srrg2_solver arithmetic, selectable per call.  0 everywhere
   * (what memset gives) = the shipped family, the one under which all 17 pose bounds of the reference's gtests hold
   * (DESIGN.md section 2).  The other values are the readings a maintainer with the real srrg2_solver sources may need instead
   * ("Which upstream lines decide the a13 forms"); the CPU checker switches the same forms (orc_set_variant). */
  int32_t kernel_weight_form;      /* RobustifierSaturated, chi > chi_threshold: PRS_KERNEL_WEIGHT_INV_CHI Omega / chi (shipped);
                                      PRS_KERNEL_WEIGHT_TAU_OVER_CHI Omega * chi_threshold / chi (the form of the in-repo smoother,
                                      mapping/landmarks/landmark_estimator_pose_based_smoother_impl.cpp:81-84) */
  int32_t damping_form;            /* IterationAlgorithmGN: PRS_DAMPING_DIAG (H + damping diag(H)) dx = -b (shipped);
                                      PRS_DAMPING_IDENTITY (H + damping I) dx = -b */
  int32_t translation_weight_form; /* aligner_slice_processor_projective.cpp:107-112, dn = d / mean disparity:
                                      PRS_TRANSLATION_WEIGHT_OFFSET min(0.01 + dn, 1) (shipped, the literal "(0.01+d,1)*I");
                                      PRS_TRANSLATION_WEIGHT_CLAMP clamp(dn, 0.01, 1).  Non-finite results count as 1 (0.01 for a NaN
                                      under CLAMP). */
  /* OPT-IN, does LESS work than the reference (MultiAligner3DQR has no termination criterion in kitti.conf:1006-1009 / euroc.conf:
   * every frame runs max_iterations): > 0 = leave the loop once the finder has latched (has_converged: the correspondences are
   * frozen) and a Gauss-Newton step's 6-vector dx = (translation, normalised quaternion part) has |dx| below this bound.  The
   * correspondence vector is the full run's (it froze before the exit); the pose differs from the max_iterations pose by about the
   * last step (with lambda = 1 on diag(H) the steps halve: |dx| < 1e-5 leaves ~1e-5).  0 (what memset gives) = off. */
  float step_norm_exit;
} prs_aligner_params;
enum { PRS_KERNEL_WEIGHT_INV_CHI = 0, PRS_KERNEL_WEIGHT_TAU_OVER_CHI = 1 };
enum { PRS_DAMPING_DIAG = 0, PRS_DAMPING_IDENTITY = 1 };
enum { PRS_TRANSLATION_WEIGHT_OFFSET = 0, PRS_TRANSLATION_WEIGHT_CLAMP = 1 };

/* The normal equations of one linearisation.  Every one of the 29 sums (21 entries of the upper triangle of H, 6 of b,
 * the two chi) is a FIXED-SHAPE float reduction over the correspondence vector (BUILD-DEFINED: the upstream factor loop
 * and its summation order live in srrg2_solver and are not pinned by anything in the reference tree; the shape is the
 * "LDS tree-reduced" one the hot path is specified with, chosen so that gfx950 evaluates it with register exchanges):
 *   leaf l (0..127)  = ((+0 + t_l) + t_{l+128}) + t_{l+256} + ...   terms of the correspondences l, l + 128, ... in order
 *   seven levels      v[l] <- v[l] + v[l ^ m]  for m = 32, 16, 8, 7, 2, 1, 64 (a balanced binary tree over the 128 leaves)
 *   sum               = v[0] + 0.0f
 * What is summed (round 4) are the CAMERA-FRAME normal equations: with [R | t] the transform a point goes through and
 * D = d(image point) / d(point in camera), J = D R [ wt I | -2 [p]x ] = D G_c Rt with G_c = [ wt I | -[y]x ], y = 2 R p and
 * Rt = blockdiag(R, R) -- the same for every correspondence --, so the terms are those of G_c^T (D^T Omega D) G_c and
 * G_c^T D^T Omega e, and H = Rt^T (sum) Rt, b = Rt^T (sum) is evaluated ONCE per linearisation on the summed system (row by
 * row; the lower triangle of the rotated matrix is the system and is mirrored).  Operation order: csrc/align.hip
 * factor_accumulate, csrc/prs_se3.h rotate_normal_equations; restated in oracle/proslam_oracle.c.
 * Same inputs give the same bits on every launch, batch size and entry point (fused, split, prs_pcf_linearize). */
typedef struct {
  float H[36];          /* last linearisation, row-major, without prior */
  float b[6];           /* sum J^T Omega e */
  float chi_inliers;
  float chi_total;
  float mean_disparity; /* value used by the factor */
  int32_t num_inliers;
  int32_t num_outliers;
  int32_t num_invalid;
  int32_t num_correspondences;
  int32_t status;       /* 1 Success, 0 Fail (tests/test_aligners.cpp:117-121) */
  int32_t iterations;   /* aligner iterations accounted for (= max_iterations in align mode) */
  int32_t iterations_executed; /* < iterations when stop_at_fixed_point cut the loop */
  int32_t warnings;     /* OR of PRS_WARN_* over the call, or a PRS_ERR_* code */
} prs_align_result;

enum {
  PRS_MODE_ALIGN     = 0, /* per iteration: finder.compute(); setupFactor; linearize; GN step */
  PRS_MODE_FINDER    = 1, /* ONE CorrespondenceFinderProjective::compute() with local_map_in_sensor = X */
  PRS_MODE_LINEARIZE = 2  /* ONE linearisation at X of the correspondences passed in */
};

/* device-resident batch of B independent frames (one per sequence).
 * fixed:  [batch][fixed_stride][4] floats: (u,v,-,-) mono, (u,v,d,-) depth, (uL,vL,uR,vR) stereo
 * moving: [batch][moving_stride][4] floats: (x,y,z, information scale of the point:
 *         1 + log(numberOfOptimizations) if > 2 else 1, aligner_slice_processor_projective.cpp:46-52)
 * Alignment (the widest piece the kernels move an array in; csrc/align.hip): fixed, moving, fixed_desc and moving_desc 16 bytes -- a
 * row of fixed / moving is one float4, a descriptor row two 16-byte halves; PRS_ERR_UNSUPPORTED otherwise, nothing launched and
 * nothing written --, state 8 (its uint64_t members), every other array 4, inputs_changed 1.
 * Extent: every array has batch (x stride) whole rows.  Of frame b the kernels read rows [0, n_fixed[b]) of fixed and fixed_desc and
 * rows [0, n_moving[b]) of moving and moving_desc (counts clamped to [0, stride]); rows from the count to the stride are never read.
 * corr: rows [0, n_corr[b]) are read where the vector is an input (PRS_MODE_LINEARIZE, a finder with nothing new to do); rows
 * [0, n_fixed[b]) may be written (a frame has at most one correspondence per fixed point, and an earlier iteration's vector may
 * have been longer than the final one); rows from n_fixed[b] to the stride are neither read nor written. */
typedef struct {
  int32_t batch;
  int32_t fixed_stride;
  int32_t moving_stride;
  const float* fixed;            /* 16-byte aligned */
  const uint8_t* fixed_desc;     /* [batch][fixed_stride][32], 16-byte aligned */
  const int32_t* n_fixed;        /* [batch] */
  const float* moving;           /* 16-byte aligned */
  const uint8_t* moving_desc;    /* [batch][moving_stride][32], 16-byte aligned */
  const int32_t* n_moving;       /* [batch] */
  const uint8_t* inputs_changed; /* [batch] setFixed/setMoving since the last call; NULL = all changed */
  prs_pcf_state* state;          /* [batch] in/out, 8-byte aligned */
  float* X;                      /* [batch][16] in: movingInFixed guess, out: estimate (row-major 4x4); read and written by element */
  prs_corr* corr;                /* [batch][fixed_stride] in/out: the caller-owned CorrespondenceVector; 4-byte aligned */
  int32_t* n_corr;               /* [batch] in/out */
  prs_align_result* result;      /* [batch], 4-byte aligned */
  const float* prior;            /* optional [batch][42]: additive H0 (36) and b0 (6) (an externally linearised slice) */
  const float* prior_mean;       /* optional [batch][16]: mean Z of the motion prior (NULL = identity) */
  int32_t max_fixed;             /* 0 = fixed_stride; else an upper bound on n_fixed[] the kernel sizes its LDS
                                    for (fewer bytes per frame = more frames per CU); a frame exceeding it
                                    gets PRS_ERR_CAPACITY in result[].warnings */
} prs_align_batch;

/* mode PRS_MODE_FINDER and PRS_MODE_LINEARIZE only enqueue.  mode PRS_MODE_ALIGN alternates a search launch and a Gauss-Newton
 * launch over the frames that are still pending (4-5 rounds at kitti.conf settings) and BLOCKS until the batch is done
 * (= prs_align_batch_enqueue + prs_align_batch_finish); results are complete in device memory when it returns. */
/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): the search launch has a workgroup of 512 threads a frame, batch <= 2^23 - 1 (the fused kernel: 256 threads,
 * 2^24 - 1).  prs_align_batch_enqueue alike. */
PRS_API int prs_align_batch_run(prs_context* ctx,
                                const prs_pcf_params* finder,
                                const prs_aligner_params* aligner,
                                const prs_align_batch* batch,
                                int32_t mode);
/* The two halves of mode PRS_MODE_ALIGN, for callers that pipeline (several contexts from one thread, or other work between
 * the two calls).  enqueue: `rounds` (0 = the nominal 5) x (search launch, Gauss-Newton launch) on the context's stream and
 * nothing else -- no host synchronisation, no readback; every launch skips the frames that are finished or not waiting for
 * it.  Once the context's scratch buffers exist (after a first batch of the same shape) the sequence allocates nothing and
 * can be captured in a HIP graph.  finish: one 4-byte readback; while frames are still pending (finder retries shift the
 * nominal schedule) four more rounds and another readback.  Between the two calls the context may run any OTHER operator
 * (matcher, scene clipper, extractor, brute-force matcher, merger: the enqueued batch owns its working buffers), but must not
 * start another aligner batch nor change its stream (PRS_ERR_UNSUPPORTED), and `batch`'s buffers must stay valid; the structs
 * themselves are copied.  finish without an enqueued batch is a no-op.
 * rearm: a HIP graph captured around enqueue replays the launches without passing through the host code; call rearm after
 * each graph launch so that finish performs its completion check (and its extra rounds) for the replayed batch.  The graph
 * bakes in the batch shape: a later enqueue with a larger batch may move the working buffers -- capture again after it. */
PRS_API int prs_align_batch_enqueue(prs_context* ctx,
                                    const prs_pcf_params* finder,
                                    const prs_aligner_params* aligner,
                                    const prs_align_batch* batch,
                                    int32_t rounds);
PRS_API int prs_align_batch_finish(prs_context* ctx);
PRS_API int prs_align_batch_rearm(prs_context* ctx);
/* rearm for a graph that is replayed on ANOTHER stream than the one the batch was enqueued / captured on: finish then synchronises
 * `hip_stream` (a hipStream_t) and enqueues its extra rounds there.  prs_align_batch_rearm assumes the capture stream; replaying
 * elsewhere without telling the library would let finish read the completion word before the replay has run.  Either way the
 * number of rounds the graph holds is the `rounds` the captured enqueue was called with (remembered by the context). */
PRS_API int prs_align_batch_rearm_on(prs_context* ctx, void* hip_stream);

/* ---- host, one frame: stateful finder handle mirroring the reference object -------------------
 * setFixed / setMoving / setLocalMapInSensor / compute (tests/test_correspondence_finders.cpp:314,
 * tests/test_aligners.cpp:658-666) */
typedef struct prs_pcf prs_pcf;
PRS_API int prs_pcf_create(prs_context* ctx, const prs_pcf_params* params, prs_pcf** out);
PRS_API int prs_pcf_destroy(prs_pcf* h);
PRS_API int prs_pcf_set_params(prs_pcf* h, const prs_pcf_params* params); /* flags a config change */
/* coords: [n][fixed_dim] floats */
PRS_API int prs_pcf_set_fixed(prs_pcf* h, const float* coords, int32_t fixed_dim, const uint8_t* desc, int32_t n);
/* xyz [n][3]; info_scale [n] or NULL (= 1) */
PRS_API int prs_pcf_set_moving(prs_pcf* h, const float* xyz, const float* info_scale, const uint8_t* desc, int32_t n);
PRS_API int prs_pcf_set_local_map_in_sensor(prs_pcf* h, const float* T16);
PRS_API int prs_pcf_set_search_radius(prs_pcf* h, uint64_t radius_pixels);      /* CF/..projective_base.h:82-85 */
PRS_API int prs_pcf_set_descriptor_distance(prs_pcf* h, float distance);        /* CF/..projective_base.h:94-97 */
PRS_API int prs_pcf_get_state(prs_pcf* h, prs_pcf_state* out);
/* mean Z (row-major 4x4) of the motion prior prs_pcf_align applies when prs_aligner_params.enable_motion_prior is set;
 * NULL = identity */
PRS_API int prs_pcf_set_motion_prior_mean(prs_pcf* h, const float* Z16);
/* out capacity >= n_fixed; untouched calls ("nothing new", converged) return the previous vector */
PRS_API int prs_pcf_compute(prs_pcf* h, prs_corr* out, int32_t capacity, int32_t* n_out);
/* the full per-frame loop on the handle's fixed/moving clouds (MultiAligner3DQR::compute stand-in) */
PRS_API int prs_pcf_align(prs_pcf* h,
                          const prs_aligner_params* aligner,
                          const float* X_init16,
                          const float* prior42, /* optional */
                          float* X_out16,
                          prs_corr* corr_out,
                          int32_t capacity,
                          int32_t* n_corr_out,
                          prs_align_result* result);
/* one linearisation of given correspondences on the handle's clouds (factor-level use,
 * tests/test_aligners.cpp:586-638) */
PRS_API int prs_pcf_linearize(prs_pcf* h,
                              const prs_aligner_params* aligner,
                              const float* X16,
                              const prs_corr* corr,
                              int32_t n_corr,
                              prs_align_result* result);

/* (H + damping diag(H)) dx = -b, X <- X * exp(dx) on the device (same arithmetic as the aligner loops: LDL^T without square roots,
 * csrc/prs_se3.h ldlt_solve6; H row-major, its LOWER triangle is read; a pivot that is not positive leaves X untouched) */
PRS_API int prs_gn_step(prs_context* ctx, const float* H36, const float* b6, float damping, float* X16);
/* the same with the damping form chosen (prs_aligner_params.damping_form: PRS_DAMPING_DIAG or PRS_DAMPING_IDENTITY) */
PRS_API int prs_gn_step_ex(prs_context* ctx, const float* H36, const float* b6, float damping, int32_t damping_form, float* X16);

/* Self-test of the reciprocal the aligner kernels use (csrc/prs_device.h, recip_exact: v_rcp_f32 + one Newton step in fused
 * multiply-adds where that equals the IEEE quotient, the compiler's division elsewhere): every one of the 2^32 float bit patterns
 * through the function as shipped, compared with 1.0f / x of the same device (NaNs compare equal).  counts[0] = operands that differ
 * (must be 0), counts[1] = operands that went through the short form (waves that held only operands of 2^-126 <= |x| < 2^126).
 * About a second on an MI355X; not part of the tracking path. */
PRS_API int prs_selftest_reciprocal(prs_context* ctx, uint64_t counts[2]);

/* host helper: information scale column from landmark ages
 * (aligner_slice_processor_projective.cpp:46-52: n > 2 ? 1 + log(n) : 1) */
PRS_API void prs_info_scale_from_nopt(const uint32_t* n_opt, int32_t n, float* scale);

/* ================================================================================================
 * Scene clipper
 * replaces SceneClipperProjective3D::compute (mapping/scene_clipper_projective_3d.cpp:9-67):
 * projector->setCameraPose(robot_in_local_map * sensor_in_robot) (:46), the projector keeps the
 * local-map points inside [range_min, range_max] and the canvas and returns them in the camera
 * frame together with their indices into the full scene (:53, globalIndices()); when
 * sensor_in_robot is not exactly the identity the kept points are moved to the robot frame
 * (:61-63).  Survivors keep ascending source order.  The clipped cloud has the layout of the
 * aligner's `moving` arrays, so it can be consumed in place.
 * Status per scene: PRS_WARN_EMPTY_INPUT for an empty full scene (outputs AND n_clipped left
 * untouched, like the reference :21-28), PRS_WARN_NO_PROJECTION when nothing survives (:55-58).
 * n_scene[b] above `stride` is read as `stride` (a scene owns `stride` rows of every array and no
 * row beyond them is read or written); n_scene[b] below zero is read as zero, an empty scene.
 * Rows at and past n_clipped[b] of the three output arrays are not written.
 * ============================================================================================== */
typedef struct {
  int32_t batch;                   /* independent scenes (one per sequence) */
  int32_t stride;                  /* row stride (points) of every per-scene array */
  const float* scene_xyzw;         /* [batch][stride][4] local-map points; w is carried through (information scale); this array,
                                      scene_desc, clipped_xyzw and clipped_desc are 16-byte aligned: a row moves in 16-byte pieces */
  const uint8_t* scene_desc;       /* [batch][stride][32] or NULL (then clipped_desc must be NULL too) */
  const int32_t* n_scene;          /* [batch] */
  const float* robot_in_local_map; /* [batch][16] row-major */
  float* clipped_xyzw;             /* out [batch][stride][4] */
  uint8_t* clipped_desc;           /* out [batch][stride][32] or NULL */
  int32_t* global_indices;         /* out [batch][stride]: clipped index -> full-scene index */
  int32_t* n_clipped;              /* out [batch] */
  int32_t* status;                 /* out [batch] */
  const uint32_t* scene_n_opt;     /* optional [batch][stride] numberOfOptimizations of the scene points: the clipped
                                      w column then is the aligner's information scale n > 2 ? 1 + log(n) : 1
                                      (aligner_slice_processor_projective.cpp:46-52), taken from a table the host
                                      evaluates with the same double log (n clamped to 4095) */
} prs_clip_batch;

/* device pointers, asynchronous on the context's stream */
/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): a workgroup of 256 threads a scene (128 scenes or more, or scenes of up to two tiles), batch <= 2^24 - 1;
 * fewer and longer scenes: tiles x batch workgroups, each dimension on its own. */
PRS_API int prs_scene_clip_batch(prs_context* ctx,
                                 const prs_projector* projector,
                                 const float* sensor_in_robot16, /* host */
                                 const prs_clip_batch* batch);

/* host pointers, one scene; capacity = rows available in the three output arrays (>= n) */
PRS_API int prs_scene_clip(prs_context* ctx,
                           const prs_projector* projector,
                           const float* robot_in_local_map16,
                           const float* sensor_in_robot16,
                           const float* scene_xyzw,
                           const uint8_t* scene_desc, /* or NULL */
                           int32_t n,
                           float* clipped_xyzw,
                           uint8_t* clipped_desc, /* or NULL */
                           int32_t* global_indices,
                           int32_t capacity,
                           int32_t* n_clipped);

/* ================================================================================================
 * Bijective brute-force descriptor matcher
 * replaces CorrespondenceFinderDescriptorBasedBruteforce::compute
 * (CF/correspondence_finder_descriptor_based_bruteforce_impl.cpp:8-155,157-199,247-293): all
 * N_f x N_m Hamming distances, candidates below maximum_descriptor_distance, registration pool by
 * pool (one pool per distinct distance) with the in-pool uniqueness test and Lowe's ratio on the
 * fixed AND the moving side.  Output order: ascending (response, fixed index) -- the reference's
 * std::sort by response alone (:94-97) leaves ties unspecified.
 * Status per pair of clouds: PRS_WARN_EMPTY_INPUT (:217-226), PRS_WARN_NO_MATCHES (:237-242),
 * PRS_ERR_CAPACITY when more candidates pass the threshold than candidate_capacity.
 * ============================================================================================== */
typedef struct {
  float maximum_descriptor_distance;           /* CF/..bruteforce.h:22-26 (default 50); must be <= 256 */
  float maximum_distance_ratio_to_second_best; /* CF/..bruteforce.h:27-31 (default 0.9) */
  float minimum_matching_ratio;                /* CF/..bruteforce.h:32-36; not read by compute() */
} prs_bruteforce_params;

typedef struct {
  int32_t batch;               /* independent (fixed, moving) cloud pairs */
  int32_t fixed_stride;        /* <= 8192 */
  int32_t moving_stride;       /* <= 65535 */
  const uint8_t* fixed_desc;   /* [batch][fixed_stride][32], 16-byte aligned like moving_desc: a descriptor is read as two 16-byte pieces */
  const int32_t* n_fixed;      /* [batch] */
  const uint8_t* moving_desc;  /* [batch][moving_stride][32] */
  const int32_t* n_moving;     /* [batch] */
  prs_corr* matches;           /* out [batch][min(fixed_stride, moving_stride)] */
  int32_t* n_matches;          /* out [batch] */
  int32_t* status;             /* out [batch] */
  int32_t candidate_capacity;  /* 0 = 16 * max(stride): pairs below the threshold the kernel can hold per cloud pair */
} prs_bruteforce_batch;

/* device pointers, asynchronous on the context's stream */
/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): the registration launch of the split shape has a workgroup of 1024 threads a cloud pair, batch <= 2^22 - 1;
 * the fused shapes launch no more workgroups than twice the compute units. */
PRS_API int prs_bruteforce_match_batch(prs_context* ctx,
                                       const prs_bruteforce_params* params,
                                       const prs_bruteforce_batch* batch);

/* host pointers, one pair of clouds; capacity >= min(n_fixed, n_moving) */
PRS_API int prs_bruteforce_match(prs_context* ctx,
                                 const prs_bruteforce_params* params,
                                 const uint8_t* fixed_desc,
                                 int32_t n_fixed,
                                 const uint8_t* moving_desc,
                                 int32_t n_moving,
                                 prs_corr* correspondences,
                                 int32_t capacity,
                                 int32_t* n_correspondences);

/* ================================================================================================
 * Landmark estimators + projective mergers
 * replaces MergerProjective_::compute with its RigidStereoTriangulation / RigidStereoProjectiveEKF /
 * ProjectiveDepthEKF specialisations (mapping/mergers/merger_projective_impl.cpp:8-328,
 * merger_projective_rigid_stereo_impl.cpp:8-77, .._triangulation_impl.cpp:7-39,
 * merger_projective_depth_ekf_impl.cpp:8-73) and the estimator each one drives:
 * LandmarkEstimatorWeightedMean_ (mapping/landmarks/landmark_estimator_weighted_mean_impl.cpp:7-41),
 * LandmarkEstimatorEKF_ + PointEKFBase + the stereo / depth / mono measurement models in double
 * (landmark_estimator_ekf_impl.cpp:7-82, filters/point_ekf_base.hpp:63-125,
 * filters/stereo_projective_point_ekf_impl.cpp:13-48, projective_depth_point_ekf_impl.cpp:7-36,
 * projective_point_ekf_impl.cpp:16-43), LandmarkEstimatorPoseBasedSmoother_
 * (landmark_estimator_pose_based_smoother_impl.cpp:7-148).
 * The local map lives on the device as a structure of arrays; one workgroup merges one frame into
 * one map: first-come bin blocking by correspondence order (:89-122), one estimator update per
 * surviving correspondence, then the binned addition of new landmarks (:210-305) in the
 * reference's order (bins in order of their first measurement, best disparity / depth per bin).
 * Every scene index may appear in at most one correspondence (the finder's output is bijective).
 * ============================================================================================== */
enum { PRS_EST_WEIGHTED_MEAN = 0, PRS_EST_EKF = 1, PRS_EST_SMOOTHER = 2 };
enum { PRS_MERGER_STEREO_TRIANGULATION = 0, PRS_MERGER_STEREO_EKF = 1, PRS_MERGER_DEPTH_EKF = 2 };
enum {
  PRS_ERR_HISTORY    = -7, /* a landmark's measurement history is full (max_measurements) */
  PRS_ERR_SCENE_FULL = -8, /* the map has no room for the landmarks to add */
  PRS_ERR_DUPLICATE  = -9  /* a scene index appears in two correspondences */
};

/* PointStatisticsField3D::CameraMeasurement; the two transforms of a measurement are per frame and
 * sit in the map's pose table */
typedef struct {
  float point_in_image[3];
  float point_in_camera[3];
  int32_t frame;
} prs_camera_measurement;

typedef struct {
  float sensor_in_world[12]; /* 3x4 row-major */
  float world_in_sensor[12];
} prs_frame_pose;

typedef struct {
  int32_t type;            /* PRS_EST_* */
  int32_t measurement_dim; /* 2 mono (estimator only), 3 depth, 4 stereo */
  float maximum_distance_geometry_meters_squared; /* landmark_estimator_base.hpp:21-25 */
  double minimum_state_element_covariance;        /* landmark_estimator_ekf.h:37-41 */
  double maximum_covariance_norm_squared;         /* :43-47 */
  double fx, fy, cx, cy, b_x, b_y;                /* filter calibration (setCameraMatrix / setBaseline) */
  uint32_t maximum_number_of_iterations;          /* landmark_estimator_pose_based_smoother.h:17-21 */
  float convergence_criterion_minimum_chi2_delta; /* :23-27 */
  float maximum_reprojection_error_pixels_squared; /* :29-33 */
  uint32_t minimum_number_of_measurements_for_optimization; /* :35-39 */
  float camera_matrix[9];                         /* smoother: setCameraMatrix */
} prs_estimator_params;

typedef struct {
  int32_t variant;        /* PRS_MERGER_* */
  int32_t enable_binning; /* MergerCorrespondence_::param_enable_binning */
  uint32_t number_of_row_bins, number_of_col_bins; /* merger_projective.h:47-56 */
  int32_t canvas_rows, canvas_cols;                /* projector canvas (:30-33) */
  float maximum_distance_appearance;               /* merger_projective.h:42-46 */
  uint32_t target_number_of_merges;                /* MergerCorrespondence_::param_target_number_of_merges */
  float target_merge_ratio;                        /* merger_projective.h:57-61 (warning only) */
  prs_triangulator_params triangulator;            /* stereo variants */
  float fx, fy, cx, cy;                            /* depth variant: unprojector */
  prs_estimator_params estimator;
} prs_merger_params;

typedef struct {
  int32_t n_merged;
  int32_t n_added;
  int32_t status; /* PRS_WARN_NO_MATCHES = all merge attempts failed (:141-144), PRS_WARN_LOW_RATIO = low merge
                     ratio (:145-150), or a PRS_ERR_* code */
} prs_merge_result;

/* B local maps + the frames merged into them; device pointers */
typedef struct {
  int32_t batch;
  int32_t capacity;           /* landmarks per map (row stride of the per-landmark arrays) */
  int32_t max_measurements;   /* history slots per landmark (0 = none kept: not with the smoother) */
  int32_t max_frames;         /* rows of the pose table per map */
  /* the map */
  float* coords;              /* [batch][capacity][4] xyz in the local map frame */
  uint8_t* desc;              /* [batch][capacity][32] */
  float* state;               /* [batch][capacity][4] statistics().state(), world frame */
  float* covariance;          /* [batch][capacity][9] */
  uint32_t* n_opt;            /* [batch][capacity] numberOfOptimizations */
  uint8_t* inlier;            /* [batch][capacity] */
  uint32_t* n_meas;           /* [batch][capacity] */
  prs_camera_measurement* meas; /* [batch][capacity][max_measurements] */
  prs_frame_pose* poses;      /* [batch][max_frames] */
  int32_t* n_points;          /* [batch] in/out */
  /* the frame */
  int32_t measurement_stride;
  const float* measurement;   /* [batch][measurement_stride][4] image-space points ((uL,vL,uR,vR) / (u,v,d,-)) */
  const uint8_t* measurement_desc; /* [batch][measurement_stride][32] */
  const int32_t* n_measured;  /* [batch] */
  int32_t corr_stride;
  const prs_corr* corr;       /* [batch][corr_stride]: fixed_idx -> scene, moving_idx -> measurement */
  const int32_t* n_corr;      /* [batch] */
  const int32_t* scene_index_map; /* optional [batch][capacity]: clipped index -> scene index (prs_clip_batch.global_indices) */
  const float* measurement_in_world; /* [batch][16] */
  const float* measurement_in_scene; /* [batch][16] */
  const int32_t* frame;       /* [batch] pose-table slot of this frame */
  prs_merge_result* result;   /* [batch] */
  int32_t corr_from_aligner;  /* 0: fixed_idx -> scene, moving_idx -> measurement (the merger's own convention,
                                 merger_projective_impl.cpp:60-77); 1: the vector comes straight from
                                 prs_align_batch.corr (fixed_idx -> measurement, moving_idx -> clipped scene) */
} prs_merge_batch;

/* Merges one frame into every map of the batch (asynchronous, on the context's stream).
 * Status per map (result[b].status), every map on its own: a map with an error leaves the other maps of the launch unaffected.
 *   PRS_ERR_RANGE      frame[b] outside [0, max_frames), n_points[b] outside [0, capacity], n_measured[b] < 0 or n_corr[b] < 0;
 *                      or the correspondence vector names a landmark outside [0, n_points[b]) (after scene_index_map, where one is
 *                      given) or a measurement outside [0, n_measured[b]), or a measurement that passes the appearance gate lies
 *                      outside the bin grid of the canvas.
 *   PRS_ERR_CAPACITY   n_measured[b] > measurement_stride or n_corr[b] > corr_stride (what prs_map_merge refuses on the host).
 *   PRS_ERR_DUPLICATE  a landmark appears in two correspondences.
 *     For these three the map's arrays, its pose table and n_points[b] are left exactly as they were and n_merged = n_added = 0.
 *     Counts are tested first; of several faults of one correspondence vector the FIRST in vector order is reported, as a
 *     sequential walk over the vector meets it (a duplicate counts at its second appearance).  A faulty vector is refused
 *     before any landmark is updated, so it also goes before the two codes below.
 *   PRS_ERR_HISTORY    (pose-based smoother) a landmark to update already holds max_measurements measurements.  The other
 *                      landmarks of the frame have been updated; nothing is added; n_merged counts the updates made.
 *   PRS_ERR_SCENE_FULL n_points[b] + the landmarks to add exceed capacity.  The frame's updates have been made, rows from
 *                      n_points[b] on may be overwritten, n_points[b] itself is unchanged and n_added = 0.
 *     After these two the map should be discarded or rebuilt: a sequential merger stops at the fault, this one does not.  The
 *     same holds for a measurement outside the bin grid that only the addition step meets (no correspondence names it):
 *     PRS_ERR_RANGE after the frame's updates.
 *   >= 0               PRS_WARN_NO_MATCHES / PRS_WARN_LOW_RATIO bits; n_points[b] has grown by n_added.
 * 2-D (mono) measurements carry no depth: that form only updates landmarks, also for a frame without correspondences.
 * Call-level errors (return value, nothing launched, every map untouched): PRS_ERR_NULL (a required pointer unset),
 * PRS_ERR_UNSUPPORTED (unknown merger / estimator or a combination no merger of the reference has, a bin narrower than one
 * pixel, or a bin table + scene bitmap + pose cache beyond the 160 KiB of LDS), PRS_ERR_HIP. */
/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): a workgroup of 256 threads a map, batch <= 2^24 - 1. */
PRS_API int prs_merge_batch_run(prs_context* ctx, const prs_merger_params* params, const prs_merge_batch* batch);

/* ---- host, one local map: stateful handle mirroring the reference's merger object ---------------------------------
 * setScene / setMeasurement / setCorrespondences / setMeasurementInScene / setMeasurementInWorld / compute
 * (mapping/mergers/merger_projective.h, tests/test_mergers.cpp:248-780).  The map lives on the device in the layout of
 * prs_merge_batch; every merge uploads the frame, runs the merge kernel(s) with batch = 1 and synchronises. */
typedef struct prs_map prs_map;
/* capacity: landmarks; max_measurements: history slots per landmark (0 = none; the pose-based smoother needs them);
 * max_frames: frames merged between two prs_map_clear calls (rows of the pose table); max_measured: measurements and
 * correspondences per frame */
PRS_API int prs_map_create(prs_context* ctx, int32_t capacity, int32_t max_measurements, int32_t max_frames, int32_t max_measured, prs_map** out);
PRS_API int prs_map_destroy(prs_map* h);
PRS_API int prs_map_clear(prs_map* h); /* a new local map: no landmarks, frame counter 0 */
/* grows the landmark arrays to `capacity` (no-op if already that large): every landmark, its state, covariance, counters and
 * measurement history are kept */
PRS_API int prs_map_reserve(prs_map* h, int32_t capacity);
PRS_API int prs_map_size(prs_map* h, int32_t* n_points, int32_t* frames_merged /* may be NULL */);
/* setScene with allocated statistics: coords_in_scene [n][3]; state_in_world [n][3] or NULL (= the coordinates,
 * tests/test_mergers.cpp:268-271); covariance [n][9] or NULL (zero: what statistics().allocate() leaves when no covariance is
 * set, tests/ref_mapping.py:_seed_map; points the merger creates get the identity, merger_projective_impl.cpp:319); desc [n][32]; n_opt [n] or NULL (0);
 * first_measurement [n] or NULL: the camera measurement the landmark was created from (its .frame names a pose-table row set
 * with prs_map_set_frame_pose; tests/test_mergers.cpp:425-433) */
PRS_API int prs_map_set_scene(prs_map* h,
                              const float* coords_in_scene,
                              const float* state_in_world,
                              const float* covariance,
                              const uint8_t* desc,
                              const uint32_t* n_opt,
                              const prs_camera_measurement* first_measurement,
                              int32_t n);
/* pose of an earlier frame the scene's measurements refer to; frames merged afterwards continue behind the highest row set */
PRS_API int prs_map_set_frame_pose(prs_map* h, int32_t frame, const float* sensor_in_world16);
/* MergerProjective_::compute for one frame.  measurement: [n_measured][estimator.measurement_dim] image-space points;
 * corr: fixed_idx -> scene, moving_idx -> measurement (corr_from_aligner = 0) or the aligner's vector (= 1, with
 * scene_index_map = the clipper's global indices, or NULL when the aligner ran on the whole scene).  Returns the warning
 * bits of result->status (>= 0) or a PRS_ERR_* code. */
PRS_API int prs_map_merge(prs_map* h,
                          const prs_merger_params* params,
                          const float* measurement_in_world16,
                          const float* measurement_in_scene16,
                          const float* measurement,
                          const uint8_t* measurement_desc,
                          int32_t n_measured,
                          const prs_corr* corr,
                          int32_t n_corr,
                          const int32_t* scene_index_map,
                          int32_t corr_from_aligner,
                          prs_merge_result* result);
/* the scene after merging; any output may be NULL: coords_in_scene / state_in_world [capacity][3], desc [capacity][32],
 * n_opt / inlier [capacity] */
PRS_API int prs_map_get_scene(prs_map* h,
                              int32_t capacity,
                              float* coords_in_scene,
                              float* state_in_world,
                              uint8_t* desc,
                              uint32_t* n_opt,
                              uint8_t* inlier,
                              int32_t* n_points);

/* pose bookkeeping between the aligner and the merger / next clip, on the device:
 * pose_out[b] = prediction[b] * X[b]^-1.  The clipper expresses the local map in the predicted sensor
 * frame (scene_clipper_projective_3d.cpp:46-53), so the aligner's estimate X (moving in fixed) is the
 * motion relative to the prediction; the tracker's new sensor pose in the map is prediction * X^-1.
 * All pointers are device arrays of [batch][16] row-major float; pose_out may alias prediction. */
PRS_API int prs_pose_compose_batch(prs_context* ctx, int32_t batch, const float* prediction, const float* X, float* pose_out);

/* MotionModelConstantVelocity3D (external; configurations/kitti.conf:257-260): the tracker's guess for the next pose
 * repeats the last inter-frame motion, pose_pred[b] = pose_prev1[b] * (pose_prev2[b]^-1 * pose_prev1[b]), with the
 * rotation block renormalised through its unit quaternion (the recursion amplifies rounding otherwise).  Up to 120 degrees
 * of rotation (real part w >= 0.5) the block is rebuilt from the imaginary part, w = sqrt(1 - |q|^2); beyond, that recovery
 * loses eps / (2 w) -- a milliradian a milliradian away from a half turn -- so the w of the extraction is carried instead: the
 * round trip costs a few 1e-7 rad at every angle (tests/test_pose_algebra_ref.py, profiles/pose_algebra/README.md).
 * Device arrays of [batch][16] row-major float; pose_pred may alias pose_prev2. */
PRS_API int prs_motion_predict_batch(prs_context* ctx, int32_t batch, const float* pose_prev2, const float* pose_prev1, float* pose_pred);

/* ================================================================================================
 * Intensity feature extraction
 * replaces IntensityFeatureExtractorBinned_::compute (sensor_processing/feature_extractors/
 * intensity_feature_extractor_binned.cpp:7-208, intensity_feature_extractor_base.cpp:56-95): FAST
 * keypoints with non-maximum suppression, the detection-region grid with "keep all below the
 * per-region target, else the best by response" (:47-196, in-repo, restated exactly), then one
 * 256-bit binary descriptor per keypoint.
 * The two OpenCV calls of the reference (cv::FastFeatureDetector::detect, cv::ORB::compute) are NOT part of the
 * reference tree; they are restated from OpenCV's published algorithms:
 *  - FAST-9 segment test on the 16-pixel circle of radius 3, response = largest threshold that still detects
 *    (cornerScore), strict 8-neighbour non-maximum suppression, outermost 3 pixels not examined, raster order;
 *  - cv::ORB::compute on provided keypoints: keypoints closer than 31 px (edgeThreshold) to the border are removed, no
 *    orientation (FAST keypoints carry angle -1: the pattern is used unrotated), the image is smoothed with the
 *    8-bit fixed-point GaussianBlur(7x7, sigma 2) and bit i compares the smoothed pixels of pair i of ORB's learned
 *    pattern (bit_pattern_31_).
 * With selection_order = PRS_SELECT_LIBSTDCXX this reproduces every feature / match count the reference's own tests
 * assert on its own KITTI / ICL / SceneFlow images (tests/test_ref_pins_gpu.py).  Outputs have the layout of
 * prs_stereo_batch's inputs.
 * Status per image: PRS_WARN_NO_MATCHES (no keypoints, :126-131), PRS_ERR_CAPACITY (more than max_raw_detections
 * raw detections or more features than `stride`).
 * ============================================================================================== */
/* which of several EQUAL responses survive the per-region cut (intensity_feature_extractor_binned.cpp:179-195 uses
 * std::sort with a response-only comparator, so the answer is implementation defined):
 *   PRS_SELECT_CANONICAL  ties in detection (raster) order; one bitonic sort of all detections of the image
 *   PRS_SELECT_LIBSTDCXX  the permutation GNU libstdc++'s std::sort produces: its introsort replayed by the waves of a
 *                         workgroup (only the ranges that reach a region's kept prefix); results identical to a reference
 *                         built with GCC, and since round 5 the faster of the two (profiles/r05/features_kitti_images.txt) */
enum { PRS_SELECT_CANONICAL = 0, PRS_SELECT_LIBSTDCXX = 1 };

typedef struct {
  int32_t detector_threshold;             /* intensity_feature_extractor_base.h:36-40; in [1, 254] */
  int32_t enable_non_maximum_suppression; /* :48-52 */
  int32_t target_number_of_keypoints;     /* :54-58 */
  int32_t number_of_detectors_vertical;   /* intensity_feature_extractor_binned.h:17-22 */
  int32_t number_of_detectors_horizontal; /* :23-28 */
  int32_t selection_order;                /* PRS_SELECT_* */
  int32_t max_raw_detections;             /* FAST detections per image the selection can hold: 0 = 8192, at most 32768 */
} prs_extractor_params;

/* Alignment (the widest piece the kernels move an array in; csrc/features.hip): images any (pixels are read by the byte, four at a
 * time inside a row where a tile lies inside the image), keypoints 8 bytes (a keypoint is stored as one piece), descriptors 4 (a
 * descriptor is stored in 32-bit words; give them 16 where they go on to a matcher), intensity, n_features and status 4.  Keypoints
 * below 8 or descriptors below 4: PRS_ERR_UNSUPPORTED, nothing launched and nothing written.
 * Extent: images end at the last pixel of the last row of the last image, (batch * rows - 1) * pitch + cols bytes: the pitch
 * padding is never read.  keypoints, intensity and descriptors have batch * stride whole rows, of which rows [0, n_features[b]) of
 * image b are written and no other; n_features and status have `batch` elements (the descriptor launch rounds the batch up to 8,
 * the images beyond `batch` do not exist for it). */
typedef struct {
  int32_t batch;
  int32_t rows, cols;     /* image size */
  int32_t pitch;          /* bytes between image rows (>= cols) */
  const uint8_t* images;  /* [batch][rows][pitch] 8-bit intensity, any alignment, to the last pixel */
  int32_t stride;         /* feature capacity per image = row stride of the outputs */
  prs_kp2* keypoints;     /* out [batch][stride] (u, v) = (column, row), 8-byte aligned */
  float* intensity;       /* out [batch][stride] or NULL */
  uint8_t* descriptors;   /* out [batch][stride][32], 4-byte aligned */
  int32_t* n_features;    /* out [batch] */
  int32_t* status;        /* out [batch] */
} prs_extract_batch;

/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): the ordering launch has a workgroup of 1024 threads an image, batch <= 2^22 - 1, and the descriptor launch
 * batch (rounded up to 8) * ceil(stride / 96) workgroups of 256. */
PRS_API int prs_extract_features_batch(prs_context* ctx, const prs_extractor_params* params, const prs_extract_batch* batch);

/* The order in which the reference's selection leaves ONE region's keypoints (PRS_SELECT_LIBSTDCXX): the permutation GNU
 * libstdc++'s std::sort produces for the comparator `a.response > b.response`
 * (intensity_feature_extractor_binned.cpp:182-186) on keypoints whose responses are response[0..n), in detection order.
 * order[k] = index of the keypoint that ends up at position k.  Host pointers; runs the same device code as the
 * extractor's selection (work queue over the workgroup's waves, ranges of <= 64 items in registers, heapsort at the depth
 * limit), synchronises.  Responses are 1..255 (a detected corner never scores 0: PRS_ERR_RANGE); n <= 32768. */
PRS_API int prs_selection_order(prs_context* ctx, const uint8_t* response, int32_t n, int32_t* order);

/* host pointers, one image: what an adapter's IntensityFeatureExtractorBase_::compute(const cv::Mat&) binds
 * (intensity_feature_extractor_binned.cpp:47-196): uploads the image, runs the three kernels, downloads the features,
 * synchronises.  image: rows x cols 8-bit pixels, `pitch` bytes between rows; keypoints [capacity][2] (u, v) floats,
 * intensity [capacity] or NULL, descriptors [capacity][32]; *n_features = features written.  More features than
 * `capacity` or more raw detections than max_raw_detections: PRS_ERR_CAPACITY (nothing is returned). */
PRS_API int prs_extract_features(prs_context* ctx,
                                 const prs_extractor_params* params,
                                 const uint8_t* image,
                                 int32_t rows,
                                 int32_t cols,
                                 int32_t pitch,
                                 float* keypoints,
                                 float* intensity,
                                 uint8_t* descriptors,
                                 int32_t capacity,
                                 int32_t* n_features);

/* ================================================================================================
 * Selective intensity feature extraction
 * replaces IntensityFeatureExtractorSelective_::computeKeypoints + compute (sensor_processing/feature_extractors/
 * intensity_feature_extractor_selective.cpp:45-203, intensity_feature_extractor_base.cpp:56-85): in TRACKING mode (the image
 * has projections) keypoints are detected only inside rectangles around the projections of tracked landmarks, and optionally
 * seeded in the rest of the image (appended behind them); in SEEDING mode (no projections) in the whole image or inside an
 * external mask.  Both use cv::GFTTDetector, restated from OpenCV's published algorithm (goodFeaturesToTrack, blockSize 3,
 * 3x3 Sobel, no Harris, qualityLevel 0.01, maxCorners = target_number_of_keypoints, minDistance = target_bin_width_pixels):
 *  - minimum eigenvalue of the 3x3 box-summed gradient covariance (reflect-101 borders, float), maximum over the detection
 *    mask only, values not above 0.01 * maximum set to 0, candidates = non-zero 3x3 local maxima inside the mask and 1 px
 *    inside the image, sorted by response, ties by pixel index descending (OpenCV >= 3.4's greaterThanPtr; the reference's
 *    pinned counts do not decide ties: this is the build's choice), accepted greedily when no accepted corner lies at a
 *    squared distance below minDistance^2, at most maxCorners;
 *  - descriptors as prs_extract_features_batch (cv::ORB::compute, unrotated pattern, 31-px border filter, order kept).
 *    "BRIEF-256" is cv::ORB as well in the reference's OpenCV >= 3 build without contrib (base.cpp:153-158).
 * Projection rectangles (selective.cpp:62-150): r = detection_radius + 10, (row, col) = round half away from zero of (v, u);
 * rows [max(row - r, 0), + min(2r, rows - that)); columns likewise, or [0, col) with enable_full_distance_to_left only,
 * [col, cols) with _right only, all columns with both.  The seeding run after tracking uses the complement of their union,
 * its own maximum and its own maxCorners budget.  Projections must lie inside the image (the reference asserts it):
 * PRS_ERR_RANGE otherwise.
 * Status per image: PRS_WARN_NO_MATCHES (no keypoints, selective.cpp:145-150,184-189), PRS_ERR_CAPACITY (more GFTT
 * candidates of one run than max_candidates, or more features than `stride`; no features are returned).
 * ============================================================================================== */
enum { PRS_DETECTOR_GFTT = 0, PRS_DETECTOR_FAST = 1 /* not built: PRS_ERR_UNSUPPORTED */ };
enum { PRS_DESCRIPTOR_ORB_256 = 0, PRS_DESCRIPTOR_BRIEF_256 = 1 };

typedef struct {
  int32_t detector_type;                 /* PRS_DETECTOR_* (intensity_feature_extractor_base.h param detector_type) */
  int32_t descriptor_type;               /* PRS_DESCRIPTOR_* (param descriptor_type) */
  int32_t target_number_of_keypoints;    /* GFTT maxCorners, per run; in [1, 8192] */
  int32_t target_bin_width_pixels;       /* GFTT minDistance; 0 = no distance test */
  int32_t enable_full_distance_to_left;  /* intensity_feature_extractor_selective.h:17-28 (default 0) */
  int32_t enable_full_distance_to_right; /* (default 0) */
  int32_t enable_seeding_when_tracking;  /* :29-34 (default 1) */
  int32_t max_candidates;                /* GFTT candidates per run the selection sort holds: 0 = 8192, at most 16384 */
} prs_selective_extractor_params;

/* Alignment (csrc/selective.hip, and csrc/features.hip for the outputs): images and seeding_mask any (read by the byte), projections
 * and keypoints 8 bytes (a prs_kp2 moves as one piece), descriptors 4 (stored in 32-bit words), every other array 4.  Projections or
 * keypoints below 8, descriptors below 4: PRS_ERR_UNSUPPORTED, nothing launched and nothing written.
 * Extent: images and seeding_mask end at the last pixel of the last row of the last image; the pitch padding is never read, and
 * the mask of an image in tracking mode is not read at all.  projections has batch * projection_stride rows, of which rows
 * [0, n_projections[b]) of image b are read; detection_radius[b] is read only where image b has projections.  The outputs as in
 * prs_extract_batch: rows [0, n_features[b]) of image b are written and no other. */
typedef struct {
  int32_t batch;
  int32_t rows, cols;           /* image size, each in [8, 4096] */
  int32_t pitch;                /* bytes between image rows (>= cols) */
  const uint8_t* images;        /* [batch][rows][pitch] 8-bit intensity, any alignment, to the last pixel */
  int32_t projection_stride;    /* row stride of projections (0 when projections is NULL) */
  const prs_kp2* projections;   /* [batch][projection_stride] (u, v) or NULL = every image seeds; 8-byte aligned */
  const int32_t* n_projections; /* [batch] projections of image b (0 = seeding mode), or NULL with projections */
  const int32_t* detection_radius; /* [batch] radius of image b's projections (setProjections), or NULL = 0 */
  const uint8_t* seeding_mask;  /* [batch][rows][pitch], non-zero = detect, used in seeding mode only (setKeypointDetectionMask);
                                   NULL = none; any alignment, to the last pixel */
  int32_t stride;               /* feature capacity per image = row stride of the outputs */
  prs_kp2* keypoints;           /* out [batch][stride] (u, v) = (column, row), 8-byte aligned */
  float* intensity;             /* out [batch][stride] or NULL */
  uint8_t* descriptors;         /* out [batch][stride][32], 4-byte aligned */
  int32_t* n_features;          /* out [batch] */
  int32_t* status;              /* out [batch] */
} prs_selective_extract_batch;

/* device pointers; enqueues on the context's stream (graph-capturable, like prs_extract_features_batch) */
/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): the selection launch has a workgroup of 512 threads an image and side, batch <= 2^23 - 1, and the descriptor
 * launch batch (rounded up to 8) * ceil(stride / 96) workgroups of 256. */
PRS_API int prs_extract_features_selective_batch(prs_context* ctx, const prs_selective_extractor_params* params,
                                                 const prs_selective_extract_batch* batch);

/* host pointers, one image: uploads, runs, downloads, synchronises (like prs_extract_features).  projections [n_projections][2]
 * (u, v) or NULL; seeding_mask rows x cols (pitch `pitch`) or NULL.  Returns the image's status; on an error nothing is returned. */
PRS_API int prs_extract_features_selective(prs_context* ctx,
                                           const prs_selective_extractor_params* params,
                                           const uint8_t* image,
                                           int32_t rows,
                                           int32_t cols,
                                           int32_t pitch,
                                           const float* projections,
                                           int32_t n_projections,
                                           int32_t detection_radius,
                                           const uint8_t* seeding_mask,
                                           float* keypoints,
                                           float* intensity,
                                           uint8_t* descriptors,
                                           int32_t capacity,
                                           int32_t* n_features);

/* ================================================================================================
 * RGB-D preprocessing: depth images to (u, v, d) measurements
 * replaces RawDataPreprocessorMonocularDepth::compute + _readDepth (sensor_processing/raw_data_preprocessor_monocular_depth.cpp:
 * 50-180) after its feature extractor has run (a separate launch behind prs_extract_features_batch or
 * prs_extract_features_selective_batch, whose outputs it reads in place).  For every feature i of an image, in order:
 *  - raw = depth(rint(v_i), rint(u_i)) (:165-166; rint rounds half to even, so -0.5 is row / column 0), a TYPE_16UC1 image read
 *    as float (exact) or a TYPE_32FC1 image (:117-129);
 *  - the feature is kept iff raw > 0 (:169: NaN, -0, 0 and negative depths are dropped, +inf is kept) with
 *    d = depth_scaling_factor_to_meters * raw (one float multiply, :170);
 *  - the kept features are compacted in order (:171-176): fixed[k] = (u, v, d, 0) with the feature's descriptor and intensity.
 * The reference does not check the lookup's bounds (undefined behaviour there): a rounded keypoint outside the depth image is
 * PRS_ERR_RANGE for that image here.
 * Status per image: the extractor's error when extract_status[b] < 0; else PRS_ERR_CAPACITY (n_features[b] > stride),
 * PRS_ERR_RANGE (a keypoint outside the depth image, or n_features[b] < 0); else the OR of PRS_WARN_NO_MATCHES (nothing kept:
 * the reference's _status = Error, :131-136; also what the extractor reports for an image without keypoints) and
 * PRS_WARN_SPARSE_DEPTH ((float) without_depth / (float) n > 0.25, :139-145).  An image with an error has n_fixed 0 and
 * outputs that are not valid; the other images of the batch are unaffected.
 * Call-level errors: PRS_ERR_UNSUPPORTED (unknown depth_type; fixed, fixed_desc or descriptors not 16-byte aligned -- a descriptor
 * moves as two 16-byte pieces --, keypoints not 8-byte aligned, depth not aligned to its element), PRS_ERR_RANGE
 * (non-finite scale, rows or cols below 1, stride below 1, pitch below cols * element size or not a multiple of it),
 * PRS_ERR_NULL (a required pointer unset, or exactly one of intensity / fixed_intensity set).
 * ============================================================================================== */
enum { PRS_DEPTH_U16 = 0, PRS_DEPTH_F32 = 1 };  /* TYPE_16UC1 / TYPE_32FC1 (:117-129) */
enum { PRS_WARN_SPARSE_DEPTH = 64 };            /* > 25 % of the features without depth (:139-145) */

typedef struct {
  int32_t depth_type;                     /* PRS_DEPTH_* (the reference takes it from the image) */
  float depth_scaling_factor_to_meters;   /* raw_data_preprocessor_monocular_depth.h:26-30 (default 1.0) */
} prs_depth_params;

typedef struct {
  int32_t batch, rows, cols, pitch;       /* depth image size; pitch in bytes, a multiple of the element size */
  const void* depth;                      /* [batch][rows][pitch] */
  int32_t stride;                         /* row stride of every per-feature array below, in and out */
  const prs_kp2* keypoints;               /* [batch][stride] (u, v): the extractor's output; 8-byte aligned */
  const float* intensity;                 /* [batch][stride] or NULL */
  const uint8_t* descriptors;             /* [batch][stride][32], 16-byte aligned */
  const int32_t* n_features;              /* [batch] */
  const int32_t* extract_status;          /* the extractor's per-image status, or NULL; may alias `status` */
  float* fixed;                           /* out [batch][stride][4] (u, v, d, 0): the layout of prs_align_batch.fixed and
                                             prs_merge_batch.measurement, consumed in place */
  uint8_t* fixed_desc;                    /* out [batch][stride][32] */
  float* fixed_intensity;                 /* out [batch][stride]; NULL iff intensity is NULL */
  int32_t* n_fixed;                       /* out [batch] */
  int32_t* status;                        /* out [batch] */
} prs_depth_batch;

/* device pointers; enqueues one kernel on the context's stream (graph-capturable, like prs_extract_features_batch).  Inputs and
 * outputs must not overlap, except extract_status with status.  A workgroup of 256 threads an image: a batch beyond 2^24 - 1 is
 * PRS_ERR_UNSUPPORTED (prs_launch_fits). */
PRS_API int prs_depth_measurements_batch(prs_context* ctx, const prs_depth_params* params, const prs_depth_batch* batch);

/* host pointers, one image: what an adapter's compute() binds.  depth: rows x cols elements of params->depth_type, `pitch` bytes
 * between rows; keypoints [n][2] (u, v), intensity [n] or NULL, descriptors [n][32]; out: uvd [n][3] (u, v, d), intensity_out
 * [n] (ignored when intensity is NULL, may be NULL), desc_out [n][32], *n_fixed.  Uploads, runs, downloads, synchronises;
 * returns the image's status (on an error nothing is returned and *n_fixed is 0). */
PRS_API int prs_depth_measurements(prs_context* ctx, const prs_depth_params* params, const void* depth, int32_t rows, int32_t cols,
                                   int32_t pitch, const float* keypoints, const float* intensity, const uint8_t* descriptors,
                                   int32_t n, float* uvd, float* intensity_out, uint8_t* desc_out, int32_t* n_fixed);

/* ================================================================================================
 * Loop aligner: point-to-point SE(3) registration of matched 3D clouds (the consumer of the
 * brute-force matcher's correspondences)
 * replaces MultiAligner3DQR "loop_aligner" with one AlignerSliceProcessor3D (registration/aligner_slice_processor_3d.hpp:7-22:
 * SE3Point2PointErrorFactor, information I3; registered at registration/instances.cpp:28,52), the aligner every shipped .conf wires
 * in as MultiLoopDetectorHBST3D.relocalize_aligner (kitti.conf:938-978), and the accept / reject verdict of the loop detector and
 * MultiRelocalizer3D (parameter comments kitti.conf:966-977).  The candidate search in front of it is the place database below, the
 * consumer of an accepted closure the pose-graph optimiser and the closure merger at the end of this header.
 *
 * The factor, the robustifiers, the loop and the verdict live in srrg2_solver / srrg2_slam_interfaces, not in the tree
 * (BUILD-DEFINED, stated like rows a13 / a14 of SURVEY.md Appendix A):
 *   factor       e = R p + t - f, X = [R | t] = movingInFixed, p a moving point, f its fixed partner; chi = e^T e (Omega = I3);
 *                J = R [I3 | -2 [p]x], the right perturbation X <- X exp(dx) of VariableSE3QuaternionRight.
 *   robustifier  inlier iff chi <= chi_threshold.  CLAMP: an outlier gets weight 0.  SATURATED: an outlier gets Omega / chi (the
 *                shipped a13 reading, PRS_KERNEL_WEIGHT_INV_CHI).  Both report an outlier's chi as chi_threshold in chi_total.  A
 *                correspondence whose chi is not finite (NaN / inf coordinates) is INVALID: no weight, neither inlier nor outlier.
 *   step         prs_gn_step's LDL^T of (H + damping diag(H)) dx = -b, X <- X exp(dx); a non-positive pivot leaves X untouched.
 *   loop         max_iterations x (linearise, step), no termination criterion; the result holds the LAST linearisation (H, b,
 *                chi sums, counts), status = num_inliers >= min_num_inliers.  n_corr < min_num_correspondences, or no
 *                correspondence at all, means status 0, no iteration and X unchanged.
 *   verdict      accepted = status && num_inliers >= relocalize_min_inliers
 *                && (float) num_inliers / (float) n_corr >= relocalize_min_inliers_ratio
 *                && chi_inliers / (float) num_inliers <= relocalize_max_chi_inliers.
 * Sums (BUILD-DEFINED, fixed shape): with y = R p (each component ((R_i0 px + R_i1 py) + R_i2 pz)), e = (y + t) - f,
 * chi = (e0 e0 + e1 e1) + e2 e2 and w the weight, the 18 terms w, w y, w (y1 y1 + y2 y2), w (y0 y0 + y2 y2), w (y0 y0 + y1 y1),
 * w (y0 y1), w (y0 y2), w (y1 y2), w e, w (y x e), chi (inliers) and chi or chi_threshold (all valid) of correspondence k go to
 * lane k mod 64, each lane sums its correspondences in ascending k from +0, and the 64 lane sums are combined by the butterfly
 * v[l] <- v[l] + v[l ^ m], m = 32, 16, 8, 4, 2, 1.  The camera-frame system [[sum w I, -2 [sum w y]x], [2 [sum w y]x,
 * 4 sum w [y]x^T[y]x]], [sum w e; 2 sum w (y x e)] is rotated once, H = Rt^T H_c Rt, b = Rt^T b_c (Rt = blockdiag(R, R)), in the
 * operation order of rotate_normal_equations with separate multiplies and adds (csrc/point_align.hip).  Same inputs give the same
 * bits for every batch size, position in the batch, kernel instantiation and entry point.
 * Checked per pair (written to result[].warnings, other pairs unaffected): a negative match_status is passed through without
 * iterating; n_corr > corr_stride, n_fixed > fixed_stride or n_moving > moving_stride gives PRS_ERR_CAPACITY, a negative count or
 * an index outside [0, n_fixed) / [0, n_moving) PRS_ERR_RANGE; zero correspondences PRS_WARN_NO_MATCHES.
 * ============================================================================================== */
/* result of one cloud pair */
typedef struct {
  float H[36];                 /* last linearisation, row-major */
  float b[6];
  float chi_inliers;
  float chi_total;
  int32_t num_inliers;
  int32_t num_outliers;
  int32_t num_invalid;
  int32_t num_correspondences; /* n_corr */
  int32_t status;              /* 1 Success, 0 Fail */
  int32_t accepted;            /* the loop detector's verdict */
  int32_t iterations;          /* linearisations run (max_iterations, 1 with linearize_only, 0 when not iterated) */
  int32_t warnings;            /* PRS_WARN_NO_MATCHES, or a PRS_ERR_* code (a negative match_status passed through) */
} prs_point_align_result;

enum { PRS_ROBUSTIFIER_CLAMP = 0, PRS_ROBUSTIFIER_SATURATED = 1 };

typedef struct {
  int32_t robustifier;                /* PRS_ROBUSTIFIER_*: RobustifierClamp / RobustifierSaturated of the slice (kitti.conf:649-677) */
  float chi_threshold;                /* the robustifier's chi_threshold */
  float damping;                      /* IterationAlgorithmGN damping of the aligner's solver (0 in every shipped .conf) */
  int32_t max_iterations;             /* MultiAligner3DQR max_iterations (one GN iteration each) */
  int32_t min_num_inliers;            /* MultiAligner3DQR min_num_inliers: status */
  int32_t min_num_correspondences;    /* AlignerSliceProcessor3D min_num_correspondences */
  int32_t relocalize_min_inliers;     /* verdict thresholds of the loop detector / MultiRelocalizer3D (kitti.conf:966-977) */
  float relocalize_min_inliers_ratio;
  float relocalize_max_chi_inliers;
  int32_t linearize_only;             /* 1: ONE linearisation at X and no step (factor-level use); 0: the aligner loop */
  int32_t parked_per_lane;            /* 0 (what memset gives) = by corr_stride; 1, 4, 6 select the kernel instantiation that
                                         keeps that many correspondences per lane in registers (tests, A-B runs: same results) */
} prs_point_align_params;

/* device-resident batch of B independent (fixed, moving) cloud pairs; rows as the triangulator and the map write them */
typedef struct {
  int32_t batch;
  int32_t fixed_stride;
  int32_t moving_stride;
  int32_t corr_stride;           /* <= 8192 (the brute-force matcher's output stride min(fixed_stride, moving_stride) fits) */
  const float* fixed;            /* [batch][fixed_stride][4] (x, y, z, -), 16-byte aligned */
  const int32_t* n_fixed;        /* [batch] */
  const float* moving;           /* [batch][moving_stride][4] (x, y, z, -), 16-byte aligned */
  const int32_t* n_moving;       /* [batch] */
  const prs_corr* corr;          /* [batch][corr_stride]: fixed_idx / moving_idx, as prs_bruteforce_match_batch emits them */
  const int32_t* n_corr;         /* [batch] */
  const int32_t* match_status;   /* optional [batch]: the matcher's status words; a negative one is passed through */
  float* X;                      /* [batch][16] in: movingInFixed guess, out: estimate (row-major 4x4) */
  prs_point_align_result* result; /* [batch] */
  uint8_t* inlier_mask;          /* optional [batch][corr_stride]: 1 = inlier at the last linearisation, 0 = outlier or invalid
                                    (0 for every correspondence of a pair that was not linearised; untouched on an error) */
} prs_point_align_pairs;

/* device pointers, asynchronous on the context's stream: one kernel launch, no allocation and no synchronisation (graph-capturable).
 * Replaces MultiAligner3DQR::compute with AlignerSliceProcessor3D (registration/aligner_slice_processor_3d.hpp:7-22) for B pairs. */
/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): a wave a pair, four pairs a workgroup of 256 threads: ceil(batch / 4) <= 2^24 - 1. */
PRS_API int prs_point_align_batch(prs_context* ctx, const prs_point_align_params* params, const prs_point_align_pairs* batch);

/* host pointers, one pair: what an adapter's compute() binds (AlignerSliceProcessor3D setFixed / setMoving / setCorrespondences,
 * MultiAligner3DQR setMovingInFixed / compute / status / movingInFixed).  fixed_xyz [n_fixed][3], moving_xyz [n_moving][3], corr
 * [n_corr] (n_corr <= 8192), X16 in/out, inlier_mask [n_corr] or NULL.  Uploads, runs, downloads, synchronises; returns the pair's
 * warnings, or its PRS_ERR_* code. */
PRS_API int prs_point_align(prs_context* ctx, const prs_point_align_params* params, const float* fixed_xyz, int32_t n_fixed,
                            const float* moving_xyz, int32_t n_moving, const prs_corr* corr, int32_t n_corr, float* X16,
                            prs_point_align_result* result, uint8_t* inlier_mask);

/* ================================================================================================
 * Loop detector: place database and candidate search (the step in front of the brute-force matcher + loop aligner chain)
 * replaces CorrespondenceFinderHBST_::compute (registration/correspondence_finders/correspondence_finder_hbst.cpp:5-91, correspondences
 * :95-127), the finder of the MultiLoopDetectorHBST3D every shipped .conf wires in (kitti.conf:938-978), and its addPreviousQuery.
 *
 * SUBSTITUTION (BUILD-DEFINED): the reference searches an srrg_hbst::BinaryTree256 (leaf size, depth and partitioning parameters),
 * an external library that is not in the tree.  This build searches the database EXHAUSTIVELY: every stored descriptor within the
 * threshold counts, a superset of what any tree returns.  The search is O(database size) per query, where a tree is sublinear, and
 * match counts and correspondence counts are >= (in general different from) HBST's.  maximum_leaf_size, maximum_depth and
 * maximum_partitioning are read from the configurations but unused.  Everything around database.match is restated exactly:
 *   Valid        only query points whose status is Valid take part (:57-62); `valid` [n] nonzero = Valid, NULL = all Valid.
 *   index_query  the number of stored maps for a new map, the stored index when the query's graph id is in the database (:47-55).
 *   match        a (query point, stored descriptor) pair with Hamming distance d < maximum_descriptor_distance (strict).
 *   age          std::fabs(index_query - reference) > minimum_age_difference_to_candidates with uint64_t operands (:73-74): when a
 *                re-queried map is older than a reference the difference wraps around and the rule passes.
 *   inliers      number_of_matches > relocalize_min_inliers (strict, :77), the count over every matching pair of the map (a
 *                negative relocalize_min_inliers compares as a huge unsigned value: nothing passes).
 *   candidates   in ascending reference (map) index (HBST's MatchVectorMap order is not in the tree: BUILD-DEFINED).
 *   correspondences of a candidate: for each stored descriptor of the map that matched, the query point with the smallest distance,
 *                the earlier query point on a tie (strict < in query order, :101-119): (fixed_idx = query point index, moving_idx
 *                = the reference's point index, response = distance), in ascending moving_idx.  The ambiguity filter
 *                object_references.size() == 1 is a no-op: every shipped .conf has maximum_distance_for_merge 0, nothing is merged.
 * Storage: a map keeps its Valid descriptors (and xyz) in point order, padded to a multiple of 16 rows.  Adding a graph id that is
 * already stored is refused (PRS_ERR_RANGE).  Status per query (status[]): PRS_WARN_EMPTY_INPUT for n_query == 0 (the reference's
 * "query descriptor vector is empty", :13-18: no candidates); PRS_ERR_RANGE for a negative graph id or n_query; PRS_ERR_CAPACITY
 * for n_query > query_stride (no candidates) or for more candidates than max_candidates (the first max_candidates are written).
 * ============================================================================================== */
typedef struct prs_place_db prs_place_db;

typedef struct {
  float maximum_descriptor_distance;              /* match iff distance < this */
  uint32_t minimum_age_difference_to_candidates;  /* kitti 10, icl 1, euroc 5 */
  int32_t relocalize_min_inliers;                 /* candidate iff number of matches > this */
  int32_t max_candidates;                         /* candidate slots per query, [1, 256] */
} prs_place_params;

/* device-resident batch of B queries and their outputs */
typedef struct {
  int32_t batch;
  int32_t query_stride;        /* rows per query slot, <= 65536 */
  const uint8_t* desc;         /* [batch][query_stride][32] */
  const uint8_t* valid;        /* optional [batch][query_stride]: nonzero = POINT_STATUS::Valid */
  const float* xyz;            /* [batch][query_stride][4] (x, y, z, -): read by prs_place_gather_pairs only */
  const int32_t* n_query;      /* [batch] */
  const int64_t* graph_id;     /* [batch] graph id of the query's local map (>= 0) */
  int32_t count_stride;        /* >= stored maps */
  uint32_t* match_counts;      /* out [batch][count_stride]: matches per stored map, before the age and inlier rules */
  int32_t key_stride;          /* >= stored rows (prs_place_db_size) */
  uint32_t* best_keys;         /* out [batch][key_stride] per stored row: distance << 23 | query point index of its best match, ~0 none */
  int32_t corr_stride;         /* >= the largest stored map (prs_place_db_size max_map_rows) */
  int32_t* candidates;         /* out [batch][max_candidates]: map indices, ascending, -1 past n_candidates */
  int32_t* n_candidates;       /* out [batch] */
  prs_corr* corr;              /* out [batch][max_candidates][corr_stride] */
  int32_t* n_corr;             /* out [batch][max_candidates] */
  int32_t* status;             /* out [batch] */
  int64_t* index_query;        /* optional out [batch] */
} prs_place_queries;

/* the pair slots (query b, candidate k) -> slot b * max_candidates + k of a loop-closure batch (prs_bruteforce_batch +
 * prs_point_align_pairs): fixed = the query's Valid points in point order, moving = the candidate map's stored points, X = identity;
 * a slot without a candidate gets n_fixed = n_moving = 0 (a query with PRS_ERR_CAPACITY for too many candidates fills its slots) */
typedef struct {
  int32_t fixed_stride;        /* >= query_stride */
  int32_t moving_stride;       /* >= the largest stored map */
  float* fixed_xyz;            /* [slots][fixed_stride][4] */
  uint8_t* fixed_desc;         /* [slots][fixed_stride][32] */
  int32_t* n_fixed;            /* [slots] */
  float* moving_xyz;           /* [slots][moving_stride][4] */
  uint8_t* moving_desc;        /* [slots][moving_stride][32] */
  int32_t* n_moving;           /* [slots] */
  float* X;                    /* [slots][16] */
} prs_place_pairs;

PRS_API int prs_place_db_create(prs_context* ctx, prs_place_db** db);
PRS_API int prs_place_db_destroy(prs_place_db* db);
PRS_API int prs_place_db_clear(prs_place_db* db);
/* device capacity for `maps` maps and `rows` stored rows (pads included); prs_place_db_add grows it on demand */
PRS_API int prs_place_db_reserve(prs_place_db* db, int64_t maps, int64_t rows);
PRS_API int prs_place_db_size(const prs_place_db* db, int32_t* maps, int32_t* rows, int32_t* max_map_rows);
/* addPreviousQuery: stores a local map (host pointers: xyz [n][3] or NULL, desc [n][32], valid [n] or NULL) as map index = the
 * number of maps stored before it; uploads and synchronises */
PRS_API int prs_place_db_add(prs_place_db* db, int64_t graph_id, const float* xyz, const uint8_t* desc, const uint8_t* valid, int32_t n);
/* device pointers, asynchronous on the context's stream: three kernel launches, no allocation and no synchronisation
 * (graph-capturable; a captured query holds the database's buffers and size as they were at capture -- prs_place_bank below keeps
 * its sizes on the device) */
PRS_API int prs_place_query_batch(prs_place_db* db, const prs_place_params* params, const prs_place_queries* queries);
/* host pointers, one query: candidates [max_candidates], corr [max_candidates][corr_stride], n_corr [max_candidates], match_counts
 * [maps] or NULL.  Returns the query's status. */
PRS_API int prs_place_query(prs_place_db* db, const prs_place_params* params, int64_t graph_id, const uint8_t* desc, const uint8_t* valid,
                            int32_t n, int32_t* candidates, int32_t* n_candidates, prs_corr* corr, int32_t corr_stride, int32_t* n_corr,
                            uint32_t* match_counts);
/* device pointers, asynchronous: after prs_place_query_batch, fill the pair slots of a loop-closure batch (one kernel launch) */
/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): a wave a (query, candidate) slot, four slots a workgroup of 256 threads: ceil(batch * max_candidates / 4)
 * <= 2^24 - 1.  prs_place_query_batch keeps its stricter 65535 queries. */
PRS_API int prs_place_gather_pairs(prs_place_db* db, const prs_place_params* params, const prs_place_queries* queries,
                                   const prs_place_pairs* pairs);

/* ------------------------------------------------------------------------------------------------
 * Place bank: B independent place databases, one per sequence, whose contents AND sizes live on the device.  The reference keeps one
 * tree per SLAM instance (MultiLoopDetectorHBST3D, correspondence_finder_hbst.cpp:47-74); a prs_place_db shared by a batch would let
 * sequence 3 find sequence 5's maps and compare positions in an interleaved list.  Query b searches database b only, a finished map
 * is stored by a kernel from the session's hand-over slots (prs_session_batch.handover_*), and nothing is sized on the host after
 * creation: a captured step sees the maps stored by earlier replays.  prs_place_db_* is unchanged and keeps serving the one-sequence
 * adapters and the plugin.
 *   arenas       fixed at creation, per sequence the arrays of a prs_place_db: desc [row_stride][32], xyz [row_stride][4], row_pidx
 *                [row_stride], tile_map [row_stride / 16], map_off / map_rows / map_gid [map_stride]; counters n_maps, n_rows,
 *                max_map_rows [batch]; node_of_map [batch][map_stride] int32, -1 where nothing is stored.  row_stride is rounded up
 *                to a multiple of 16 (a 16-row tile never spans two maps).
 *   append       prs_place_db_add on the device (addPreviousQuery), one workgroup per sequence: the Valid rows in point order on the
 *                arena's tail, padded with zero rows (row_pidx -1) to a multiple of 16; xyz is stored as (x, y, z, 0), zeros
 *                without xyz.  After an append the arena holds what prs_place_db_add builds from the same rows, so queries are
 *                bit-equal.  node_of_map = (int32) (graph_id - graph_id_base[b]) (base 0 without the array).  Per sequence
 *                (status[]), nothing written and the counters unchanged in every case, tested in this order: n_query == 0
 *                PRS_WARN_EMPTY_INPUT (the session's "no split this frame"); a negative n_query or graph id PRS_ERR_RANGE; n_query >
 *                query_stride PRS_ERR_CAPACITY; a graph id already stored IN THIS SEQUENCE PRS_ERR_RANGE; n_maps == map_stride or
 *                n_rows + padded rows > row_stride PRS_ERR_CAPACITY.  n_query > 0 without a Valid row stores a map of 0 rows.
 *   query        every rule of the block comment above with the sequence's own indices; sizes are read from the counters.  The
 *                grids are sized by capacity, workgroups past the live sizes return at once.  match_counts [0, n_maps[b]) and
 *                best_keys [0, n_rows[b]) of query b are written, the rest is untouched.  A candidate map larger than
 *                corr_stride (a slot larger than moving_stride in the gather) is refused on the device: n_corr 0 and
 *                PRS_ERR_CAPACITY for the query (n_fixed = n_moving = 0 for the slot).
 *   links        optional outputs that let prs_pose_graph_append_closures consume the result as it stands: candidates_flat =
 *                b * map_stride + map index (-1 none), query_node = (int32) (graph_id[b] - graph_id_base[b]), -1 for a query
 *                without candidates or with an error.  The closures struct is then candidates = candidates_flat, n_maps = batch *
 *                map_stride, node_of_map = the bank's array, node_of_query = query_node, graph_of_query = 0 .. B - 1.
 * Order within a step is the reference's: query, gather, append -- a map never matches itself because it is not stored yet.  All
 * three are plain launches on the context's stream: no allocation, no synchronisation, no host read (graph-capturable).
 * Call-level (return value, nothing launched): PRS_ERR_NULL (a struct or mandatory pointer unset); PRS_ERR_RANGE (batch differs from
 * the bank's); PRS_ERR_UNSUPPORTED (query_stride outside [1, 65536]; rows not aligned: 4 bytes for the query's descriptors, 16 for
 * append and gather); PRS_ERR_CAPACITY
 * (count_stride < map_stride, key_stride < row_stride, corr_stride or moving_stride < min(row_stride, the largest query_stride
 * prs_place_bank_append_batch has accepted so far): the live sizes are not known on the host, so the capacities decide).
 * ---------------------------------------------------------------------------------------------- */
typedef struct prs_place_bank prs_place_bank;

/* the maps to store, shaped like the session's hand-over slots and the first fields of prs_place_queries (device pointers) */
typedef struct {
  int32_t batch;                 /* == the bank's */
  int32_t query_stride;          /* rows per slot, <= 65536 */
  const uint8_t* desc;           /* [batch][query_stride][32], 16-byte aligned */
  const uint8_t* valid;          /* optional [batch][query_stride]: nonzero = Valid; NULL: all Valid */
  const float* xyz;              /* optional [batch][query_stride][4] (x, y, z, -), 16-byte aligned; NULL: zeros are stored */
  const int32_t* n_query;        /* [batch]; 0: nothing to store */
  const int64_t* graph_id;       /* [batch] */
  const int64_t* graph_id_base;  /* optional [batch]: node_of_map = graph_id - base */
  int32_t* status;               /* out [batch] */
} prs_place_bank_append;

typedef struct {
  int32_t* candidates_flat;      /* out [batch][max_candidates]: b * map_stride + map index, -1 = none */
  int32_t* query_node;           /* out [batch] */
  const int64_t* graph_id_base;  /* optional [batch] */
} prs_place_bank_links;

/* row_stride is rounded up to a multiple of 16; batch in [1, 65535], map_stride >= 1, row_stride in [1, 2^20] (PRS_ERR_RANGE) */
PRS_API int prs_place_bank_create(prs_context* ctx, int32_t batch, int32_t map_stride, int32_t row_stride, prs_place_bank** bank);
PRS_API int prs_place_bank_destroy(prs_place_bank* bank);
/* asynchronous, one launch (graph-capturable): every sequence empty, node_of_map -1 */
PRS_API int prs_place_bank_clear(prs_place_bank* bank);
/* host arrays [batch] (each may be NULL); copies the counters back and synchronises: tests and tools only */
PRS_API int prs_place_bank_sizes(prs_place_bank* bank, int32_t* maps, int32_t* rows, int32_t* max_map_rows);
/* sizeof prs_place_bank_append, prs_place_bank_links as the library was compiled (bindings check) */
PRS_API void prs_place_bank_struct_sizes(uint64_t* sizes2);
/* node_of_map lives in the caller's device array [batch][map_stride] from now on (what prs_pose_graph_closures.node_of_map reads);
 * the current contents are copied over (asynchronous).  NULL: back to the bank's own array.  The array must outlive the bank's use. */
PRS_API int prs_place_bank_bind_node_of_map(prs_place_bank* bank, int32_t* node_of_map);
/* device pointers, asynchronous on the context's stream, one launch each (prs_place_bank_query_batch: three) */
PRS_API int prs_place_bank_append_batch(prs_place_bank* bank, const prs_place_bank_append* in);
PRS_API int prs_place_bank_query_batch(prs_place_bank* bank, const prs_place_params* params, const prs_place_queries* queries,
                                       const prs_place_bank_links* links /* may be NULL */);
PRS_API int prs_place_bank_gather_pairs(prs_place_bank* bank, const prs_place_params* params, const prs_place_queries* queries,
                                        const prs_place_pairs* pairs);

/* ================================================================================================
 * Pose-graph optimiser: SE(3) graphs with loop closures (the consumer of the loop detector's accepted closures)
 * replaces the `global_solver` every shipped .conf wires into MultiGraphSLAM3D (kitti.conf:895-936 -> Solver :420-444 with
 * max_iterations 10, IterationAlgorithmGN :826-832 with damping 1e-06, SimpleTerminationCriteria :884-889 with epsilon 0.001,
 * SparseBlockLinearSolverCholeskyCholmod; closure_validator is null in every file) and the insertion of a closure
 * (query map, candidate map, X) as an edge of the graph.  The closure MERGER (landmarks of the two maps) is still not served.
 *
 * The factor, the algorithm, the criterion and the linear solver live in srrg2_solver, not in the tree (BUILD-DEFINED, stated like
 * rows a13 / a14 of SURVEY.md Appendix A and the loop aligner above).  Everything is float64 except the measurements:
 *   factor       stands in for SE3PosePoseGeodesicErrorFactor.  Edge (from, to, Z, Omega): E = Z^-1 X_from^-1 X_to (isometry
 *                inverses [R^T | -R^T t] and products in the expression order of csrc/prs_se3.h, in double), e = t2tnq(E): the
 *                translation and the imaginary part of the unit quaternion (w, v) with w >= 0; chi = e^T Omega e.  Z is float32
 *                [16] (it comes from prs_point_align_pairs.X or the tracker), Omega float32 [36] row-major, both widened exactly.
 *   perturbation X <- X tnq2t(dx) (VariableSE3QuaternionRight).  Rotations are NOT re-orthonormalised: X in must be isometries.
 *   Jacobians    with E = [R_E | t_E], A = X_from^-1 X_to = [R_A | t_A], Z = [R_Z | t_Z]:
 *                J_to = [[R_E, 0], [0, w I + [v]x]],  J_from = [[-R_Z^T, 2 R_Z^T [t_A]x], [0, -(w I - [v]x) R_Z^T]]
 *                (tests/test_pose_graph_ref.py checks both against central differences).
 *   sums         edges are taken in ascending index.  Per edge: Omega e, Omega J_from, Omega J_to (each entry a chain over the
 *                inner index, ascending, starting with its first product), then J_from^T (Omega J_from), J_to^T (Omega J_to),
 *                J_to^T (Omega J_from) -- the block (to, from); for from > to its transpose goes to block (from, to) of the lower
 *                triangle -- and J^T (Omega e), the same chains over the row index.  A diagonal block, an off-diagonal block, a
 *                segment of b and chi each add their edges' terms in ascending edge index from +0.  Separate multiplies and adds.
 *   fixed nodes  fixed[i] != 0: the node's edges add nothing to its blocks and its segment of b; its diagonal block is the
 *                identity (not damped), so dx = 0 and the pose is not touched.
 *   damping      prs_gn_step's: PRS_DAMPING_DIAG h_rr <- h_rr + damping * h_rr (shipped), PRS_DAMPING_IDENTITY h_rr + damping.
 *   solve        scalar LDL^T on the row envelope in the natural node order, no reordering: first(j) = the smallest node joined
 *                to j by an edge, or j; the six scalar rows of node j start at column 6 first(j) and envelope_blocks = sum over j of
 *                (j - first(j) + 1).  u_rc = h_rc - sum_m l_rm u_cm, l_rc = u_rc * (1 / d_c), d_r = h_rr - sum_m l_rm u_rm, every sum
 *                one chain in ascending m over the columns both rows hold; one IEEE reciprocal per pivot.  y_r = -b_r - sum_m l_rm
 *                y_m (ascending m); z = y * (1 / d); for r descending dx_r = z_r, then z_m -= l_rm dx_r for every m of row r.
 *                A pivot that is <= 0 or not finite ends the graph with PRS_ERR_NOT_POSITIVE_DEFINITE: its poses stay as they
 *                were before that iteration.  (A free node without an edge, damping 0, is such a case.  A free COMPONENT with
 *                edges but without a fixed node is singular only up to rounding: it may pass with a meaningless step; fix a node
 *                per component or damp.)
 *   loop         iteration it = 0 .. max_iterations - 1: linearise (chi[it]), test, solve, update every free node.  The test is the
 *                BUILD-DEFINED reading of SimpleTerminationCriteria's "ratio of decay of chi2 between iteration": epsilon > 0,
 *                it > 0 and chi[it-1] - chi[it] < epsilon * chi[it-1] stops before solving; epsilon <= 0 disables it.  After the
 *                last update one error-only pass writes chi_final.  max_iterations <= PRS_POSE_GRAPH_MAX_ITERATIONS.
 * Same inputs give the same bits for every batch size, position in the batch and entry point: no floating-point atomics.
 * Checked per graph (result[].status, other graphs unaffected), in this order: a negative count PRS_ERR_RANGE; n_nodes >
 * node_stride or n_edges > edge_stride PRS_ERR_CAPACITY; n_nodes == 0 PRS_WARN_EMPTY_INPUT; an endpoint outside [0, n_nodes) or
 * from == to PRS_ERR_RANGE; an envelope larger than the graph's share of the workspace PRS_ERR_CAPACITY.  No edges, or no free
 * node: success with 0 iterations.  Multiple edges between the same pair are allowed.
 * Limits: node_stride <= 1024 (PRS_ERR_CAPACITY at the call).  One wave works on a graph; it keeps 1 / d and the right-hand side
 * (6 doubles per node each), first() and the row offsets (one int per node each) in LDS, 104 bytes per node, and the block row it
 * is factorising in what is left of the 160 KiB (54 KiB, 194 blocks wide, at node_stride 1024; wider rows are factorised in place
 * in the workspace, same bits).  The envelope itself lives in the caller's workspace: 288 bytes per block.
 * ============================================================================================== */
#define PRS_POSE_GRAPH_MAX_ITERATIONS 32
enum { PRS_ERR_NOT_POSITIVE_DEFINITE = -10 }; /* a pivot of the pose graph's normal matrix is <= 0 or not finite */

typedef struct {
  float damping;             /* IterationAlgorithmGN damping (1e-06 in every shipped .conf) */
  int32_t damping_form;      /* PRS_DAMPING_DIAG (0, shipped) or PRS_DAMPING_IDENTITY */
  int32_t max_iterations;    /* Solver max_iterations (10), <= PRS_POSE_GRAPH_MAX_ITERATIONS */
  float epsilon;             /* SimpleTerminationCriteria epsilon (0.001); <= 0: no criterion */
  float closure_information; /* prs_pose_graph_append_closures: Omega = closure_information * I6 */
} prs_pose_graph_params;

typedef struct {
  double chi[PRS_POSE_GRAPH_MAX_ITERATIONS]; /* chi[it] of every linearisation, 0 past `linearizations` */
  double chi_final;                          /* after the last update */
  int32_t linearizations;                    /* entries of chi[] */
  int32_t iterations;                        /* updates applied (a run the criterion stops has linearizations = iterations + 1) */
  int32_t envelope_blocks;
  int32_t status;                            /* PRS_OK, PRS_WARN_EMPTY_INPUT or a PRS_ERR_* code */
} prs_pose_graph_result;

/* device-resident batch of B independent graphs */
typedef struct {
  int32_t batch;
  int32_t node_stride;       /* <= 1024 */
  int32_t edge_stride;
  int32_t reserved;
  double* X;                 /* [batch][node_stride][16] in: guess, out: estimate (row-major 4x4 isometries), 8-byte aligned */
  const uint8_t* fixed;      /* [batch][node_stride] */
  const int32_t* n_nodes;    /* [batch] */
  int32_t* from;             /* [batch][edge_stride] (written by prs_pose_graph_append_closures only) */
  int32_t* to;               /* [batch][edge_stride] */
  float* Z;                  /* [batch][edge_stride][16] measurement: X_from^-1 X_to */
  float* omega;              /* [batch][edge_stride][36] row-major, or NULL: identity for every edge */
  int32_t* n_edges;          /* [batch] in; in/out for prs_pose_graph_append_closures */
  void* workspace;           /* the envelopes: workspace_bytes / batch per graph (prs_pose_graph_workspace_bytes) */
  uint64_t workspace_bytes;
  prs_pose_graph_result* result; /* [batch] */
} prs_pose_graphs;

/* the loop detector's outputs for B queries of max_candidates slots each (ops.LoopDetectorBatch: prs_place_queries.candidates,
 * prs_point_align_pairs.result and .X) and where they go.  DIRECTION: prs_place_gather_pairs makes the query the fixed cloud and the
 * candidate map the moving one, and the aligner's X is movingInFixed (e = R p + t - f, p a moving point): X = X_query^-1 X_candidate.
 * The appended edge is therefore from = the query's node, to = the candidate map's node, Z = X. */
typedef struct {
  int32_t n_queries;
  int32_t max_candidates;
  int32_t n_maps;                       /* entries of node_of_map */
  int32_t reserved;
  const int32_t* candidates;            /* [n_queries][max_candidates] map indices, -1 = none */
  const prs_point_align_result* result; /* [n_queries * max_candidates]: accepted != 0 selects the slot */
  const float* X;                       /* [n_queries * max_candidates][16] */
  const int32_t* graph_of_query;        /* [n_queries] target graph; outside [0, batch): the query is skipped */
  const int32_t* node_of_query;         /* [n_queries] node of the query's local map; < 0: skipped */
  const int32_t* node_of_map;           /* [n_maps] node of every stored map; < 0: slots of that map are skipped */
  int32_t* status;                      /* out [batch]: PRS_OK, PRS_ERR_CAPACITY (nothing appended to that graph), PRS_ERR_RANGE */
  int32_t* n_appended;                  /* optional out [batch] */
} prs_pose_graph_closures;

/* bytes of workspace for `batch` graphs whose envelopes hold up to envelope_blocks_per_graph 6 x 6 blocks each (288 bytes a block;
 * a chain of n nodes has 2 n - 1, a closure (i, j) adds |j - i| - 1 unless a longer one already ends at the same node) */
PRS_API uint64_t prs_pose_graph_workspace_bytes(int32_t batch, int32_t node_stride, int64_t envelope_blocks_per_graph);
/* sizeof prs_pose_graph_params, _result, prs_pose_graphs, prs_pose_graph_closures as the library was compiled (bindings check) */
PRS_API void prs_pose_graph_struct_sizes(uint64_t* sizes4);
/* device pointers, asynchronous on the context's stream: one kernel launch, no allocation and no synchronisation (graph-capturable) */
/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): a wave a graph, batch <= 2^26 - 1; prs_pose_graph_append_closures and prs_pose_graph_optimize_lm_batch alike. */
PRS_API int prs_pose_graph_optimize_batch(prs_context* ctx, const prs_pose_graph_params* params, const prs_pose_graphs* graphs);
/* device pointers, asynchronous, one kernel launch: appends the accepted closures to the graphs' edge lists, per graph in ascending
 * slot order (a prefix count, not arrival order).  A graph whose edge_stride would overflow gets PRS_ERR_CAPACITY and nothing.
 * graphs->omega == NULL requires closure_information == 1 (PRS_ERR_UNSUPPORTED otherwise). */
PRS_API int prs_pose_graph_append_closures(prs_context* ctx, const prs_pose_graph_params* params, const prs_pose_graphs* graphs,
                                           const prs_pose_graph_closures* closures);
/* host pointers, one graph of up to 1024 nodes: what an adapter's compute() binds.  X16 [n_nodes][16] double in/out, fixed [n_nodes],
 * from / to [n_edges], Z16 [n_edges][16] float, omega36 [n_edges][36] float or NULL.  Sizes the envelope, uploads, runs, downloads,
 * synchronises; returns the graph's status. */
PRS_API int prs_pose_graph_optimize(prs_context* ctx, const prs_pose_graph_params* params, int32_t n_nodes, double* X16,
                                    const uint8_t* fixed, int32_t n_edges, const int32_t* from, const int32_t* to, const float* Z16,
                                    const float* omega36, prs_pose_graph_result* result);

/* ------------------------------------------------------------------------------------------------
 * Levenberg-Marquardt form of the optimiser above: what icl.conf:665-685 and tum.conf:174-194 wire into their global_solver
 * (IterationAlgorithmLM: lm_iterations_max 100, step_high 0.666667, step_low 0.333333, tau 1e-05, user_lambda_init 0,
 * variable_damping 1).  IterationAlgorithmLM lives in srrg2_solver, not in the tree: BUILD-DEFINED like the rest of this section.
 * The reading is Nielsen's gain-ratio schedule as g2o implements it, which is what the .conf comments describe ("upper / lower
 * clamp for lambda if things go well", "tau: scale factor for the lambda computed by the system", "variable_damping: lambda *
 * diag(H), otherwise lambda * I").  Factor, Jacobians, sums, fixed nodes, solve, pose update and the per-graph checks are those of
 * prs_pose_graph_optimize_batch (the same device functions); the Gauss-Newton entry points are not touched by any of this.
 *   state        lambda and nu, double, per graph.  The float parameters are widened once.
 *   round        it = 0 .. max_iterations - 1:
 *                1 linearise at X: chi[it], H, b.
 *                2 the stop test of the Gauss-Newton loop, unchanged (chi[] holds accepted states only).
 *                3 it == 0: nu = 2; lambda = user_lambda_init if that is > 0, else tau * max h_rr over the scalar rows of free
 *                  nodes (a maximum has no order).  In the second case a maximum that is not > 0, or a h_rr of a free node that is
 *                  not finite, ends the graph with PRS_ERR_NOT_POSITIVE_DEFINITE, poses untouched, no trial.
 *                4 keep d_r = h_rr (undamped), g_r = -b_r and X0 = X (workspace, 28 doubles per node behind the envelope).
 *                5 trials t = 1 .. lm_iterations_max:
 *                  a damp: h_rr + lambda * h_rr (variable_damping != 0) or h_rr + lambda: the two damping forms above with lambda
 *                    for `damping`; fixed nodes the identity; right-hand side -b.  For t > 1 the undamped system is linearised
 *                    again at X0 (the same bits; no second envelope is kept).
 *                  b solve as above.  A pivot <= 0 or not finite: the trial is rejected (e), X is untouched.
 *                  c X <- X0 tnq2t(dx) for free nodes; chi_t by the error-only pass.
 *                  d scale = (sum over the scalar rows r of free nodes of dx_r * ((lambda * D_r) * dx_r + g_r)) + 1e-3, D_r = d_r
 *                    (variable_damping != 0) or 1: separate multiplies and adds, ONE chain over r ascending from +0, the 1e-3 added
 *                    last.  rho = (chi[it] - chi_t) / scale, one IEEE division.  (The sum is the decrease of the linearised chi,
 *                    without a factor 1/2; the 1e-3 is g2o's guard against 0 / 0.)
 *                  e accept iff rho > 0 and chi_t is finite: u = 2 * rho - 1, alpha = 1 - (u * u) * u, lambda <- lambda *
 *                    max(step_low, min(alpha, step_high)), nu <- 2, the round ends.  Otherwise X <- X0, lambda <- lambda * nu,
 *                    nu <- 2 * nu, and a lambda that is no longer finite ends the trials.
 *                6 a round with an accepted trial is an iteration.  A round without one ends the run with the poses X0:
 *                  PRS_ERR_NOT_POSITIVE_DEFINITE if its last trial failed on a pivot, else PRS_OK with stalled = 1.
 *                After the last round one error-only pass writes chi_final.
 *   consequences a graph whose optimum has zero residual (a tree) reaches chi = 0, which the stop test does not catch
 *                (0 - 0 < epsilon * 0 is false); every later trial is rejected (rho = 0) until lambda overflows after about 45
 *                trials: stalled = 1, PRS_OK, poses restored -- harmless.  A free node that no edge reaches has h_rr = 0: with
 *                variable_damping != 0 every trial fails on its pivot (PRS_ERR_NOT_POSITIVE_DEFINITE after lm_iterations_max
 *                trials or when lambda overflows); with variable_damping == 0 the graph solves.
 * Same inputs give the same bits for every batch size, position in the batch and entry point.  Per-graph checks and limits as
 * above, with the envelope's room = the graph's share of the workspace less 28 doubles per node of node_stride (a workspace sized
 * by prs_pose_graph_workspace_bytes is too small: PRS_ERR_CAPACITY).  At the call: lm_iterations_max < 1 or step_low > step_high,
 * a parameter that is not finite, tau < 0 or max_iterations outside [0, 32] PRS_ERR_RANGE.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  float user_lambda_init;    /* > 0: the first lambda; otherwise tau * max h_rr (0 shipped) */
  float tau;                 /* 1e-05 */
  float step_high;           /* 0.666667 */
  float step_low;            /* 0.333333 */
  int32_t lm_iterations_max; /* trials per round (100), >= 1 */
  int32_t variable_damping;  /* != 0: lambda * diag(H) (shipped), 0: lambda * I */
  int32_t max_iterations;    /* Solver max_iterations (10): rounds, <= PRS_POSE_GRAPH_MAX_ITERATIONS */
  float epsilon;             /* SimpleTerminationCriteria epsilon (0.001); <= 0: no criterion */
} prs_pose_graph_lm_params;

typedef struct {
  double chi[PRS_POSE_GRAPH_MAX_ITERATIONS];     /* chi[it] of every round's linearisation, 0 past `linearizations` */
  double chi_final;                              /* at the poses returned */
  double lambda[PRS_POSE_GRAPH_MAX_ITERATIONS];  /* the lambda the round's last trial solved with; 0 for rounds without a trial */
  int32_t trials[PRS_POSE_GRAPH_MAX_ITERATIONS]; /* trials of every round */
  int32_t linearizations;                        /* entries of chi[] (linearisations repeated for t > 1 are not counted) */
  int32_t iterations;                            /* rounds with an accepted trial */
  int32_t envelope_blocks;
  int32_t status;                                /* PRS_OK, PRS_WARN_EMPTY_INPUT or a PRS_ERR_* code */
  int32_t trials_total;
  int32_t rejected_not_positive_definite;        /* trials rejected at a pivot */
  int32_t stalled;                               /* 1: the last round accepted no trial and did not fail on a pivot */
  int32_t reserved;
} prs_pose_graph_lm_result;

/* bytes of workspace for the LM entry: the envelopes as above and 28 doubles per node of node_stride per graph */
PRS_API uint64_t prs_pose_graph_lm_workspace_bytes(int32_t batch, int32_t node_stride, int64_t envelope_blocks_per_graph);
/* sizeof prs_pose_graph_lm_params, prs_pose_graph_lm_result as the library was compiled (bindings check) */
PRS_API void prs_pose_graph_lm_struct_sizes(uint64_t* sizes2);
/* device pointers, asynchronous on the context's stream: one kernel launch, no allocation and no synchronisation (graph-capturable).
 * `graphs` as for prs_pose_graph_optimize_batch with a workspace of prs_pose_graph_lm_workspace_bytes; graphs->result is ignored and
 * may be NULL: results go to result [batch] (device, 8-byte aligned). */
PRS_API int prs_pose_graph_optimize_lm_batch(prs_context* ctx, const prs_pose_graph_lm_params* params, const prs_pose_graphs* graphs,
                                             prs_pose_graph_lm_result* result);
/* host pointers, one graph: prs_pose_graph_optimize with the LM loop */
PRS_API int prs_pose_graph_optimize_lm(prs_context* ctx, const prs_pose_graph_lm_params* params, int32_t n_nodes, double* X16,
                                       const uint8_t* fixed, int32_t n_edges, const int32_t* from, const int32_t* to, const float* Z16,
                                       const float* omega36, prs_pose_graph_lm_result* result);

/* ================================================================================================
 * Closure merger: folds the landmarks of the local map being left into the one a relocalisation re-enters
 * replaces MergerCorrespondencePointIntensityDescriptor3f, the `closure_merger` of every shipped tracker slice (kitti.conf:446-460,
 * euroc.conf:519, icl.conf:773, tum.conf:437, malaga.conf:536; apps/app_benchmark.cpp:140-160 setClosure, :183 merge), and
 * MergerCorrespondenceProjectiveDepth3D, the same merger behind an unprojection
 * (mapping/mergers/merger_correspondence_projective_depth_3d.cpp:7-33; tests/test_mergers.cpp:174-246).
 *
 * BUILD-DEFINED: MergerCorrespondence_::compute lives in srrg2_slam_interfaces, which is not in the tree.  The rule below is this
 * build's, fitted to the two results the reference pins for the base merge on its ICL frames (321 points stay 321 and nothing moves;
 * 321 become 431 with 338 measurements, every old point within 0.25 per coordinate); tests/closure_merge_ref.py restates it in
 * numpy float32 and the kernel equals that bit for bit.  Float expressions are evaluated term by term, left to right.
 *   1 points      an XYZ measurement (x, y, z, -) is used as is; a (u, v, d, -) measurement is unprojected, p = ((u - cx) / fx * d,
 *                 (v - cy) / fy * d, d), the expression of PRS_MERGER_DEPTH_EKF.  A measurement with a component of p that is not
 *                 finite, or (u, v, d) with d <= 0, is invalid: never merged, never added.
 *   2 merge       per correspondence, in any order (the result does not depend on it): skipped if response >= maximum_response or the
 *                 measurement is invalid; q = measurement_in_scene * p; d2 = (dx dx + dy dy) + dz dz against the landmark; skipped
 *                 unless d2 < maximum_distance_geometry_squared; else coords = 0.5f * (coords + q) (the row's fourth float is kept),
 *                 the landmark takes the measurement's descriptor (merger_projective_impl.cpp:186) and the measurement is marked
 *                 merged.  Every landmark a correspondence names gets inlier = merged ? 1 : 0 (:66), a merged one n_opt += 1 and,
 *                 where the map keeps it, state = (scene_in_world * coords, 0).  n_merged counts merged correspondences.
 *   3 how many    n_to_add = max(0, min(target_number_of_merges - n_merged, n_measured - n_merged)) if n_merged <
 *                 target_number_of_merges, else 0 (:158-163).
 *   4 candidates  the valid measurements that were not merged.  At most n_to_add of them: all are added.  Otherwise, without binning,
 *                 the first n_to_add in measurement order.
 *   5 binning     decides only WHICH candidates are taken when there are more than n_to_add.  Image position: (u, v) of a (u, v, d)
 *                 measurement; u = fx * x / z + cx, v = fy * y / z + cy of an XYZ measurement with z > 0.  A point whose position is
 *                 not inside [0, canvas_cols) x [0, canvas_rows) is unbinned.  bin_row = round(v / (canvas_rows / number_of_row_bins)),
 *                 the column likewise (:32-35, :84-85, std::round).  Bins that hold a merged measurement are blocked.  Pass 1 takes,
 *                 per unblocked bin, the candidate with the smallest depth (p.z), the lowest index on ties; of more than n_to_add
 *                 winners the lowest measurement indices are kept.  Pass 2 fills what is left from the remaining candidates, unbinned
 *                 ones included, in measurement order.
 *   6 append      the chosen measurements in ascending measurement index from row n_points: coords = (q, 0), the descriptor copied;
 *                 where the map keeps them state = (scene_in_world * q, 0), covariance identity, n_opt = 0, inlier = 1, n_meas = 0
 *                 (:317-320).  n_points grows by n_added.
 * Status per pair (result[b].status), every pair on its own:
 *   PRS_ERR_RANGE      n_points[b] outside [0, capacity], n_measured[b] < 0 or n_corr[b] < 0; or a correspondence names a landmark
 *                      outside [0, n_points[b]) or a measurement outside [0, n_measured[b]).
 *   PRS_ERR_CAPACITY   n_measured[b] > measurement_stride or n_corr[b] > corr_stride.
 *   PRS_ERR_DUPLICATE  a landmark appears in two correspondences.
 *     For these three the pair is left exactly as it was and n_merged = n_added = 0.  Counts are tested first; of several faults of
 *     one vector the FIRST in vector order is reported (a duplicate counts at its second appearance).
 *   PRS_ERR_SCENE_FULL n_points[b] + n_added > capacity (n_points[b] + n_added == capacity fits).  Decided before anything is
 *                      appended: the merges of step 2 have been made, no row from n_points[b] on is written, n_points[b] is unchanged,
 *                      n_merged is reported and n_added = 0.
 *   PRS_OK             otherwise; also for a pair whose gate says "not accepted", which is left exactly as it was (0 merged, 0 added).
 * Limits (PRS_ERR_UNSUPPORTED at the call, nothing launched): measurement_stride <= 16384; the scene bitmap (capacity / 8 bytes), the
 * measurement bitmaps (4.5 bytes per 8 measurements of measurement_stride) and the bin table (8 bytes per bin of (rows + 2) x
 * (cols + 2)) share 64 KiB of LDS; with binning 1 .. 4096 bins a side and a canvas; coords, desc, state, measurement and
 * measurement_desc 16-byte aligned.  PRS_ERR_NULL: a required pointer unset, or state without scene_in_world.
 * ============================================================================================== */
enum { PRS_CLOSURE_XYZ = 0, PRS_CLOSURE_UVD = 1 };

typedef struct {
  int32_t measurement_kind;  /* PRS_CLOSURE_XYZ: MergerCorrespondencePointIntensityDescriptor3f; _UVD: ..ProjectiveDepth3D */
  int32_t enable_binning;    /* MergerCorrespondence_::param_enable_binning (1 in every shipped .conf) */
  uint32_t number_of_row_bins, number_of_col_bins; /* 10, 30 (merger_projective.h:47-56) */
  int32_t canvas_rows, canvas_cols;
  float fx, fy, cx, cy;      /* the unprojector's (UVD) / the binning projection's (XYZ) camera matrix */
  float maximum_distance_geometry_squared; /* 0.25 */
  float maximum_response;                  /* 50 */
  uint32_t target_number_of_merges;        /* 200 */
} prs_closure_merger_params;

/* B (scene, measurement) pairs; device pointers */
typedef struct {
  int32_t batch;
  int32_t capacity;            /* landmarks per scene (row stride of the per-landmark arrays) */
  /* the scene: required */
  float* coords;               /* [batch][capacity][4] xyz in the scene frame */
  uint8_t* desc;               /* [batch][capacity][32] */
  int32_t* n_points;           /* [batch] in/out */
  /* its statistics: each optional, NULL if not kept */
  float* state;                /* [batch][capacity][4] world frame; needs scene_in_world */
  float* covariance;           /* [batch][capacity][9] */
  uint32_t* n_opt;             /* [batch][capacity] */
  uint8_t* inlier;             /* [batch][capacity] */
  uint32_t* n_meas;            /* [batch][capacity] */
  const float* scene_in_world; /* [batch][16] */
  /* the measurement cloud */
  int32_t measurement_stride;
  int32_t corr_stride;
  const float* measurement;    /* [batch][measurement_stride][4]: (x, y, z, -) or (u, v, d, -) */
  const uint8_t* measurement_desc; /* [batch][measurement_stride][32] */
  const int32_t* n_measured;   /* [batch] */
  const prs_corr* corr;        /* [batch][corr_stride] */
  const int32_t* n_corr;       /* [batch] */
  const float* transform;      /* [batch][16] */
  const prs_point_align_result* gate; /* optional [batch]: a pair whose `accepted` is 0 is left untouched */
  prs_merge_result* result;    /* [batch] */
  int32_t corr_from_aligner;   /* 0: fixed_idx -> scene, moving_idx -> measurement; 1: the aligner's / matcher's vector
                                  (fixed_idx -> measurement, moving_idx -> scene), as in prs_merge_batch */
  int32_t transform_is_scene_in_measurement; /* 0: transform is measurement_in_scene; 1: its rigid inverse is taken.  The loop
                                  aligner's X is movingInFixed with the query fixed: with the candidate map as the scene and the
                                  query as the measurement, X is scene-in-measurement */
} prs_closure_merge_batch;

/* device pointers, asynchronous on the context's stream: one kernel launch, no allocation and no synchronisation (graph-capturable) */
/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): a workgroup of 256 threads a map, batch <= 2^24 - 1. */
PRS_API int prs_closure_merge_batch_run(prs_context* ctx, const prs_closure_merger_params* params, const prs_closure_merge_batch* batch);
/* sizeof prs_closure_merger_params, prs_closure_merge_batch as the library was compiled (bindings check) */
PRS_API void prs_closure_merge_struct_sizes(uint64_t* sizes2);
/* host pointers, one pair, arrays of `capacity` rows in the layout above (coords4 / state4 [capacity][4]; any of state4 ..
 * n_meas may be NULL; measurement4 [n_measured][4]).  Uploads, runs, downloads, synchronises; returns result->status.  n_measured
 * is the measurement_stride of the limits above: beyond them PRS_ERR_UNSUPPORTED, with result and every array as the caller left them. */
PRS_API int prs_closure_merge(prs_context* ctx, const prs_closure_merger_params* params, int32_t capacity, int32_t* n_points,
                              float* coords4, uint8_t* desc, float* state4, float* covariance9, uint32_t* n_opt, uint8_t* inlier,
                              uint32_t* n_meas, const float* scene_in_world16, const float* measurement4,
                              const uint8_t* measurement_desc, int32_t n_measured, const prs_corr* corr, int32_t n_corr,
                              int32_t corr_from_aligner, const float* transform16, int32_t transform_is_scene_in_measurement,
                              prs_merge_result* result);
/* merges a measurement cloud into a device-resident map handle (prs_map_create), whose statistics arrays are kept up;
 * measurement4 [n_measured][4]; scene_in_world16 NULL = identity.  No frame is counted and the pose table is not touched.
 * Returns result->status.  The handle's max_measured is the call's measurement_stride and corr_stride: more measurements or
 * correspondences than that is PRS_ERR_CAPACITY, and a handle created with max_measured > 16384 (or a capacity whose bitmap does
 * not fit) gets PRS_ERR_UNSUPPORTED from every call, whatever n_measured; in both cases the map is left as it was. */
PRS_API int prs_map_merge_closure(prs_map* h, const prs_closure_merger_params* params, const float* transform16,
                                  int32_t transform_is_scene_in_measurement, const float* scene_in_world16, const float* measurement4,
                                  const uint8_t* measurement_desc, int32_t n_measured, const prs_corr* corr, int32_t n_corr,
                                  int32_t corr_from_aligner, prs_merge_result* result);

/* ================================================================================================
 * Local-map manager: per-sequence splits, pose-graph growth and trajectories (the loop around the tracker)
 * replaces the bookkeeping of SLAMBenchmark::benchmarkCompute between tracker->align() and tracker->merge()
 * (apps/app_benchmark.cpp:100-183): the trajectory log (:107-121), the switch on the tracker's status (:123-178) with
 * LocalMapSplittingCriterionViewpoint3D (kitti.conf:542-550) and makeNewMap(1) / makeNewMap(0.1), and unrollFullTrajectory
 * (:195-203).  One launch per frame between prs_align_batch_run and prs_merge_batch_run; it stands where prs_pose_compose_batch,
 * the copy of the previous pose, prs_motion_predict_batch and the copies into the merger's two pose arrays stood.
 *
 * BUILD-DEFINED: makeNewMap, the MultiTracker status and the criterion class live in srrg2_slam_interfaces, which is not in the
 * tree.  The rule below is this build's; tests/session_ref.py restates it in numpy and the kernels equal that bit for bit.  Float32
 * expressions are explicit two-operand operations in the order written (csrc/prs_se3.h: se3_inverse, se3_mul, motion_predict).
 * Per sequence b, with k = n_frames[b]:
 *   frame 0      k == 0: pose = prev = I, no criterion, frame[b] = 0, n_corr_merge[b] = 0, the log gets (cur_node[b], I).  Graph b is
 *                expected to hold node 0 with X = I, fixed = 1, n_nodes = 1, n_edges = 0 and cur_node[b] = 0.
 *   pose         lost = result[b].status != 1 or result[b].warnings < 0.  Not lost: pose_new = prediction * X^-1 (the expressions of
 *                prs_pose_compose_batch).  Lost: pose_new = prediction -- a failed alignment never enters the pose (the reference's
 *                finder resets its estimate to identity on total loss).  prev_new = pose (the old one).
 *   log          before the switch, as :107-121: frame_node[b][k] = cur_node[b], frame_pose[b][k] = pose_new.  On a split frame the
 *                logged pose is relative to the OLD map.
 *   criterion    t2 = (tx tx + ty ty) + tz tz and c = (((r00 + r11) + r22) - 1) * 0.5f of pose_new.  Viewpoint split iff t2 > d2 or
 *                c < cos_a, both strict; the launcher forms d2 = local_map_distance * local_map_distance in float and cos_a =
 *                (float) cos((double) local_map_angle_distance_radians), and an angle >= pi never splits by rotation (cos_a = -inf).
 *                No acos on the device: a restatement decides the same bits.
 *   split        reason 2 (lost, information = lost_information, makeNewMap(0.1)) goes before reason 1 (viewpoint, information =
 *                split_information, makeNewMap(1)).  New node m = n_nodes[b]: X[m] = X[cur_node] * (double) pose_new (float64, the
 *                expressions of se3_mul), fixed[m] = 0; new edge n_edges[b]: from = cur_node, to = m, Z = pose_new, omega =
 *                information * I6; n_nodes++, n_edges++, cur_node = m.  Rebase: prev = pose_new^-1 * prev_new, pose = I.  The
 *                finished map is handed over (below), then reset: n_points[b] = 0, n_meas[b][0 .. capacity) = 0.  frame[b] = 0 and
 *                n_corr_merge[b] = 0: the frame's measurements seed the new map in the one merge that follows.
 *   no split     frame[b] = slot[b], n_corr_merge[b] = n_corr[b], pose = pose_new, prev = prev_new.
 *   after either slot[b] = frame[b] + 1, n_frames[b]++, prediction = the constant-velocity prediction of (prev, pose) (the function of
 *                prs_motion_predict_batch), measurement_in_world[b] = measurement_in_scene[b] = pose.
 *   hand-over    optional (handover_desc != NULL), prs_place_queries-shaped: on a split rows [0, n_points) of coords and desc are
 *                copied to handover_xyz[b] / handover_desc[b], handover_n_query[b] = n_points, handover_graph_id[b] =
 *                graph_id_base[b] (0 without the array) + the old node; with no split (or an error) handover_n_query[b] = 0, which
 *                prs_place_query_batch answers with PRS_WARN_EMPTY_INPUT and no candidates.
 * status[b] and reason[b] (PRS_SESSION_*: the split performed):
 *   PRS_ERR_RANGE     a negative n_frames, slot, cur_node, n_nodes, n_edges or n_points, cur_node >= n_nodes, n_nodes > node_stride,
 *                     n_edges > edge_stride or n_points > capacity: nothing but status, reason and handover_n_query is written.
 *   PRS_ERR_CAPACITY  a split needs a node beyond node_stride or an edge beyond edge_stride: the split is not performed (reason 0)
 *                     and the sequence goes on in its map (the no-split branch, with pose_new as computed).  Also n_frames[b] >=
 *                     frame_stride: the step runs and only the log row is skipped.
 *   PRS_OK            otherwise.  A sequence never writes outside its rows, whatever its status.
 * Call-level (return value, nothing launched): PRS_ERR_NULL (a mandatory pointer unset; handover_xyz / _n_query / _graph_id are
 * mandatory once handover_desc is set), PRS_ERR_CAPACITY (handover_stride < capacity), PRS_ERR_RANGE (a stride or capacity below 1, a
 * parameter that is not finite or a negative distance), PRS_ERR_UNSUPPORTED (coords, desc, handover_xyz or handover_desc not 16-byte
 * aligned, graph_X not 8-byte aligned, or graphs without omega and an information other than 1).
 * One 256-thread workgroup per sequence, no allocation, no synchronisation, no host read: graph-capturable.
 *
 * prs_session_unroll_batch: out[b][k] = (float) X[b][frame_node[b][k]] * frame_pose[b][k] for k < min(n_frames[b], frame_stride), float32
 * se3_mul as unrollFullTrajectory composes Isometry3f; rows from n_frames[b] on, and rows whose node is outside [0, node_stride), are
 * left untouched.  Before or after prs_pose_graph_optimize*_batch it gives the open-loop or the optimised trajectory.
 * ============================================================================================== */
enum { PRS_SESSION_NO_SPLIT = 0, PRS_SESSION_SPLIT_VIEWPOINT = 1, PRS_SESSION_SPLIT_LOST = 2 };

typedef struct {
  float local_map_distance;               /* kitti.conf:549 (10), euroc.conf:638 (1), icl.conf:553 (5), tum.conf:546 (1) */
  float local_map_angle_distance_radians; /* kitti.conf:546 (0.25), euroc.conf:635 (0.5), icl.conf:550 (3), tum.conf:543 (0.25) */
  float split_information;                /* makeNewMap(1), apps/app_benchmark.cpp:143 */
  float lost_information;                 /* makeNewMap(0.1), :167 */
} prs_session_params;

/* B sequences; device pointers.  The arrays of the aligner (prs_align_batch), the merger (prs_merge_batch) and the pose graphs
 * (prs_pose_graphs) are those structs' own arrays. */
typedef struct {
  int32_t batch;
  int32_t frame_stride;        /* log rows per sequence */
  int32_t capacity;            /* landmarks per map (prs_merge_batch.capacity) */
  int32_t node_stride;         /* prs_pose_graphs.node_stride */
  int32_t edge_stride;         /* prs_pose_graphs.edge_stride */
  int32_t handover_stride;     /* rows per hand-over slot, >= capacity */
  /* the session's own state */
  float* pose;                 /* [batch][16] sensor in the current local map */
  float* prev;                 /* [batch][16] the pose one frame earlier, in the same map */
  float* prediction;           /* [batch][16] in: the prediction the frame was aligned at; out: the next frame's */
  int32_t* slot;               /* [batch] pose-table slot the next frame of the map takes */
  int32_t* cur_node;           /* [batch] node of the current local map */
  int32_t* n_frames;           /* [batch] frames stepped */
  int32_t* frame_node;         /* [batch][frame_stride] */
  float* frame_pose;           /* [batch][frame_stride][16] */
  int32_t* status;             /* out [batch] */
  int32_t* reason;             /* out [batch] PRS_SESSION_* */
  /* the aligner's outputs */
  const float* X;              /* [batch][16] */
  const prs_align_result* result; /* [batch] */
  const int32_t* n_corr;       /* [batch] */
  /* the map and the merger's per-frame inputs */
  const float* coords;         /* [batch][capacity][4] */
  const uint8_t* desc;         /* [batch][capacity][32] */
  int32_t* n_points;           /* [batch] */
  uint32_t* n_meas;            /* [batch][capacity] */
  int32_t* frame;              /* out [batch] prs_merge_batch.frame */
  int32_t* n_corr_merge;       /* out [batch] prs_merge_batch.n_corr */
  float* measurement_in_world; /* out [batch][16] */
  float* measurement_in_scene; /* out [batch][16] */
  /* the pose graphs */
  double* graph_X;             /* [batch][node_stride][16] */
  uint8_t* fixed;              /* [batch][node_stride] */
  int32_t* n_nodes;            /* [batch] */
  int32_t* from;               /* [batch][edge_stride] */
  int32_t* to;                 /* [batch][edge_stride] */
  float* Z;                    /* [batch][edge_stride][16] */
  float* omega;                /* [batch][edge_stride][36], or NULL (both informations must be 1) */
  int32_t* n_edges;            /* [batch] */
  /* optional hand-over of a finished map to the loop detector (prs_place_queries.desc / xyz / n_query / graph_id) */
  uint8_t* handover_desc;      /* [batch][handover_stride][32] */
  float* handover_xyz;         /* [batch][handover_stride][4] */
  int32_t* handover_n_query;   /* [batch] */
  int64_t* handover_graph_id;  /* [batch] */
  const int64_t* graph_id_base; /* optional [batch] */
} prs_session_batch;

/* device pointers, asynchronous on the context's stream: one kernel launch each */
/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): a workgroup of 256 threads a sequence, batch <= 2^24 - 1; prs_session_step_archive_batch and
 * prs_session_reenter_batch alike. */
PRS_API int prs_session_step_batch(prs_context* ctx, const prs_session_params* params, const prs_session_batch* batch);
/* out [batch][frame_stride][16] */
PRS_API int prs_session_unroll_batch(prs_context* ctx, const prs_session_batch* batch, float* out);
/* sizeof prs_session_params, prs_session_batch as the library was compiled (bindings check) */
PRS_API void prs_session_struct_sizes(uint64_t* sizes2);

/* ================================================================================================
 * Map re-entry: finished local maps are archived on the device and reloaded when a closure leads back into one
 * replaces what SLAMBenchmark::benchmarkCompute does with an accepted closure at a split (apps/app_benchmark.cpp:136-160): it does
 * not open a new local map, it re-enters the old one and calls tracker->setClosure(...) ("reloading old local map"), so that the
 * closure merger (:183) folds the map being left into the one re-entered.  Two launches around the loop detector:
 *   prs_session_step_archive_batch   in the place of prs_session_step_batch: the same step, and a finished map's whole state is kept
 *   prs_session_reenter_batch        after prs_place_bank_* / prs_point_align_batch, prs_pose_graph_append_closures and the
 *                                    optimiser (the reference's order: detect, validate, optimise, relocalize), before
 *                                    prs_closure_merge_batch_run and prs_merge_batch_run
 *
 * BUILD-DEFINED: relocalize(), MultiRelocalizer3D and setClosure live in srrg2_slam_interfaces, which is not in the tree.  The rule
 * below is this build's; tests/reentry_ref.py restates it in numpy and the kernels equal that bit for bit.  Float32 expressions are
 * explicit two-operand operations in the order written (csrc/prs_se3.h: se3_inverse, se3_mul, motion_predict).
 *
 * Archive (prs_map_archive, caller-owned device arrays): per sequence slot_stride fixed slots of `capacity` rows, each the
 * per-landmark arrays of prs_merge_batch (coords [4], desc [32], state [4], covariance [9], n_opt, inlier, n_meas: 109 bytes a
 * landmark), n_points and next_frame per slot and, both or neither, the measurement history meas [capacity][max_measurements] and
 * the pose table poses [max_frames].  Per sequence slot_of_node [node_stride] (-1 = the node's map is not archived; the caller fills
 * it with -1 before the first frame), n_slots and status.
 *
 * prs_session_step_archive_batch: every output of prs_session_step_batch, bit for bit (the same kernel body behind a block-uniform
 * flag), and per sequence b:
 *   no split     (or a session status PRS_ERR_RANGE): archive.status[b] = PRS_OK, nothing else of the archive is written.
 *   split        (lost or viewpoint) before the map is reset: the slot is slot_of_node[b][old node] if that is >= 0 -- a re-entered
 *                map that is finished again overwrites its own slot -- else slot n_slots[b], with n_slots[b]++ and slot_of_node set.
 *                Rows [0, n_points) of every per-landmark array (n_meas before it is zeroed), n_points, next_frame = slot[b] as the
 *                frame found it and, where kept, rows [0, n_points) of the history and the whole pose table are copied.
 *                archive.status[b] = PRS_OK.
 *   full         n_slots[b] == slot_stride (or outside [0, slot_stride]) and the node has no slot: archive.status[b] =
 *                PRS_ERR_CAPACITY, nothing is stored, the split proceeds as without an archive.  A slot_of_node entry >= slot_stride:
 *                PRS_ERR_RANGE, nothing stored.
 * Call-level, besides prs_session_step_batch's: PRS_ERR_NULL (maps, archive or one of their arrays unset; meas without poses or the
 * reverse, in the archive or, once the archive keeps them, in maps), PRS_ERR_RANGE (batch, capacity or node_stride differ between
 * the structs, slot_stride < 1, or the archive keeps the history and max_measurements / max_frames differ from maps' or are < 1),
 * PRS_ERR_UNSUPPORTED (the archive's coords, desc or state, or maps' state, not 16-byte aligned; other arrays not 4-byte aligned).
 *
 * prs_session_reenter_batch, per sequence b, one workgroup:
 *   eligible     reason[b] == PRS_SESSION_SPLIT_VIEWPOINT (the reference never relocalises on Lost) and the session's status[b] ==
 *                PRS_OK.  Otherwise the sequence is treated as "no slot qualifies".
 *   the split    m = n_nodes[b] - 1 must be cur_node[b] and exactly one edge e of [0, n_edges[b]) must have to == m; f = from[e] is
 *                the finished map's node, Z_e the sensor pose in f.
 *   qualifies    candidate slot k of [0, max_candidates), s = b * max_candidates + k: c = candidates_flat[s] >= 0 with c - b *
 *                map_stride in [0, map_stride), result[s].accepted != 0, o = node_of_map[c] with 0 <= o < n_nodes[b], o != f, o != m
 *                and slot_of_node[b][o] >= 0; num_inliers >= relocalize_min_inliers; (float) num_inliers / (float)
 *                num_correspondences >= relocalize_min_inliers_ratio; chi_inliers / (float) num_inliers <=
 *                relocalize_max_chi_inliers; and, with P = X_s^-1 * Z_e (se3_inverse, se3_mul) and t2 = (tx tx + ty ty) + tz tz of
 *                P, t2 <= max_translation * max_translation (the product formed in float by the launcher).  Every comparison is
 *                non-strict: equality passes.  These are MultiRelocalizer3D's values (kitti.conf:100-109), not the detector's.
 *   winner       the largest num_inliers, the lowest k on a tie.  No slot qualifies: reentered[b] = 0, gate[b].accepted = 0,
 *                merge_n_corr[b] = 0, status[b] = PRS_OK and nothing of the session, the map or the graph is written.
 *   graph        edge e is removed: the edges behind it (the closures prs_pose_graph_append_closures appended this frame) move
 *                down by one in their order -- from, to, Z and, where kept, omega; n_edges--, n_nodes--, cur_node = o.  The frame
 *                log is not touched: the split frame stays logged against f.
 *   session      pose = P, prev = P * prev, prediction = motion_predict(prev, pose), measurement_in_world = measurement_in_scene =
 *                pose.
 *   map          the archive slot of o goes back into the live arrays: rows [0, n_points) of every per-landmark array, n_points,
 *                n_meas[n_points .. capacity) = 0.  With the history kept: its rows [0, n_points), the pose table, frame[b] =
 *                next_frame.  Without: n_meas = 0 everywhere and frame[b] = 0.  slot[b] = frame[b] + 1.
 *   regular merge   n_corr_merge[b] = 0 and n_measured[b] = 0: the reference runs the closure merger IN PLACE of the regular merger
 *                on this frame, so the prs_merge_batch_run that follows adds nothing to the re-entered map.
 *   closure merge   the outputs form a prs_closure_merge_batch of batch B over the live map: corr = merge_corr, n_corr =
 *                merge_n_corr (the winner's matcher vector, corr_from_aligner = 1), transform = merge_transform = X_s
 *                (transform_is_scene_in_measurement = 1), scene_in_world[b] = (float) graph_X[b][o], gate[b] = result[s] with
 *                accepted = 1; the measurement cloud is the session's hand-over slot (the finished map, PRS_CLOSURE_XYZ).
 *                INVARIANT: the vector's moving indices are rows of the map as the bank stored it, used here as rows of the map as
 *                the archive holds it.  A map's rows are only ever appended to (merger and closure merger), so the bank's
 *                first-stored version is a prefix of every later archived one and the indices name the same landmarks.
 *   status[b]    PRS_ERR_RANGE, with nothing but status[b] and reentered[b] = 0 written (gate[b] keeps what an earlier frame left:
 *                stop the sequence): an eligible sequence with n_nodes outside [1, node_stride], n_edges outside [0, edge_stride],
 *                cur_node != n_nodes - 1, not exactly one edge into m or its from outside [0, m); the winner's archive slot >=
 *                slot_stride, its n_points outside [0, capacity] or its n_corr outside [0, corr_stride].  PRS_OK otherwise.  A
 *                sequence never writes outside its rows.
 * Call-level (return value, nothing launched): PRS_ERR_NULL, PRS_ERR_RANGE (strides or the capacity differ or are < 1,
 * max_candidates < 1, a parameter not finite or negative), PRS_ERR_UNSUPPORTED (alignment, as above), as the session block's.
 * One 256-thread workgroup per sequence for both launches: a re-entry moves one map (0.4 MB at 4096 landmarks) on a frame that
 * splits, and a grid of row chunks would have to agree on the winner first (profiles/reentry/README.md).  No allocation, no
 * synchronisation, no host read: graph-capturable.
 * ============================================================================================== */
typedef struct {
  int32_t batch;
  int32_t capacity;            /* rows per slot == prs_session_batch.capacity */
  int32_t slot_stride;         /* slots per sequence */
  int32_t node_stride;         /* == prs_session_batch.node_stride */
  int32_t max_measurements;    /* with the history: == prs_merge_batch.max_measurements */
  int32_t max_frames;          /* with the history: == prs_merge_batch.max_frames */
  float* coords;               /* [batch][slot_stride][capacity][4], 16-byte aligned */
  uint8_t* desc;               /* [batch][slot_stride][capacity][32], 16-byte aligned */
  float* state;                /* [batch][slot_stride][capacity][4], 16-byte aligned */
  float* covariance;           /* [batch][slot_stride][capacity][9] */
  uint32_t* n_opt;             /* [batch][slot_stride][capacity] */
  uint8_t* inlier;             /* [batch][slot_stride][capacity] */
  uint32_t* n_meas;            /* [batch][slot_stride][capacity] */
  int32_t* n_points;           /* [batch][slot_stride] */
  int32_t* next_frame;         /* [batch][slot_stride] pose-table slot the map's next frame takes */
  prs_camera_measurement* meas; /* optional [batch][slot_stride][capacity][max_measurements] */
  prs_frame_pose* poses;       /* optional (with meas) [batch][slot_stride][max_frames] */
  int32_t* slot_of_node;       /* [batch][node_stride], -1 = none */
  int32_t* n_slots;            /* [batch] */
  int32_t* status;             /* out [batch], written by prs_session_step_archive_batch */
} prs_map_archive;

typedef struct {
  float max_translation;              /* MultiRelocalizer3D max_translation: kitti.conf:100 (10), euroc.conf:143 (2.5), icl.conf:696 (3), tum.conf:59 (1) */
  int32_t relocalize_min_inliers;     /* kitti.conf:106 (25) */
  float relocalize_min_inliers_ratio; /* kitti.conf:109 (0.5) */
  float relocalize_max_chi_inliers;   /* kitti.conf:103 (5) */
} prs_reentry_params;

/* the loop detector's outputs for B sequences of max_candidates slots each, and the kernel's own outputs; device pointers */
typedef struct {
  int32_t max_candidates;
  int32_t map_stride;                    /* the place bank's */
  int32_t corr_stride;                   /* entries per slot of corr, and per sequence of merge_corr */
  int32_t reserved;
  const int32_t* candidates_flat;        /* [batch][max_candidates] prs_place_bank_links.candidates_flat */
  const prs_point_align_result* result;  /* [batch * max_candidates] prs_point_align_pairs.result */
  const float* X;                        /* [batch * max_candidates][16] prs_point_align_pairs.X */
  const prs_corr* corr;                  /* [batch * max_candidates][corr_stride] the matcher's vectors */
  const int32_t* n_corr;                 /* [batch * max_candidates] */
  const int32_t* node_of_map;            /* [batch][map_stride] the bank's */
  int32_t* n_measured;                   /* [batch] prs_merge_batch.n_measured: zeroed on a re-entry */
  int32_t* reentered;                    /* out [batch] 1: the sequence re-entered an archived map */
  int32_t* status;                       /* out [batch] */
  prs_corr* merge_corr;                  /* out [batch][corr_stride] prs_closure_merge_batch.corr */
  int32_t* merge_n_corr;                 /* out [batch] .n_corr */
  float* merge_transform;                /* out [batch][16] .transform */
  float* scene_in_world;                 /* out [batch][16] .scene_in_world */
  prs_point_align_result* gate;          /* out [batch] .gate */
} prs_reentry_batch;

/* device pointers, asynchronous on the context's stream: one kernel launch each.  maps supplies the live map's statistics arrays
 * (state, covariance, n_opt, inlier and, with the history, meas and poses); its coords, desc, n_meas and n_points are the session's */
PRS_API int prs_session_step_archive_batch(prs_context* ctx, const prs_session_params* params, const prs_session_batch* batch,
                                           const prs_merge_batch* maps, const prs_map_archive* archive);
PRS_API int prs_session_reenter_batch(prs_context* ctx, const prs_reentry_params* params, const prs_session_batch* batch,
                                      const prs_merge_batch* maps, const prs_map_archive* archive, const prs_reentry_batch* reentry);
/* sizeof prs_map_archive, prs_reentry_params, prs_reentry_batch as the library was compiled (bindings check) */
PRS_API void prs_map_archive_struct_sizes(uint64_t* sizes3);

/* ================================================================================================
 * World map: one landmark cloud per sequence, in the world frame of the pose graph as it stands, from the archive and the live map
 * stands where SLAMBenchmark::benchmarkCompute speaks of "global landmark updates" (apps/app_benchmark.cpp:180-182), which the
 * reference performs only for the map being tracked.  Landmarks live in their local map's frame (coords); the one world-frame copy
 * is `state`, written by the merger with the scene_in_world of the merge frame, and stale as soon as prs_pose_graph_optimize*_batch
 * moves the nodes.  This call puts archive, live map and graph together on the device: it runs after the optimiser, at any frame or
 * at the end, and changes nothing it reads unless refresh_state asks for it.
 *
 * BUILD-DEFINED: the reference writes no map file, so the rule below is this build's.  tests/world_map_ref.py restates it in numpy
 * and the kernels equal that byte for byte (explicit two-operand float64 operations in the order written, -ffp-contract=off).
 *
 *   maps         per sequence b the nodes n = 0 .. n_nodes[b] - 1 in ascending order, each with at most one map.  include_live and
 *                n == cur_node[b]: the live map -- coords, desc and n_points[b] of the session, n_opt, inlier and state of `maps` --
 *                also when the node has an archive slot (a re-entered map's live copy is the newer one).  Otherwise s =
 *                slot_of_node[b][n] >= 0: archive slot s with its own n_points.  Otherwise the node contributes nothing.
 *   rows         row r of a chosen map is kept when r < n_points, n_opt[r] >= min_n_opt, (!require_inlier or inlier[r] != 0) and
 *                its three world coordinates are finite.  A row that fails the last test alone counts in n_nonfinite[b].
 *   world        with X = graph_X[b][n] (float64, row-major 4x4) and (x, y, z) = coords[r]:
 *                w_i = (float) (((X[4i+0] * (double) x + X[4i+1] * (double) y) + X[4i+2] * (double) z) + X[4i+3]), i = 0, 1, 2: one
 *                rounding to float, never through (float) X, which at kilometre translations loses the millimetres the optimiser
 *                recovered.  "Finite" is tested on the rounded floats.  The output row is (w_0, w_1, w_2, coords[r][3]), the last
 *                one copied bit for bit.
 *   order        kept rows by node ascending, then by row ascending.  Row i < out_stride of that order is written to xyz[b][i],
 *                desc[b][i], node[b][i] (n), row[b][i] (r), n_opt[b][i]; rows from n_out[b] on are left untouched.  n_total[b]
 *                counts every kept row; n_total[b] > out_stride: status[b] = PRS_ERR_CAPACITY, n_out[b] = out_stride and those rows
 *                are valid.
 *   count only   xyz == NULL: n_total, n_nonfinite and status are written, n_out[b] = 0, no other output is touched and the status
 *                is never PRS_ERR_CAPACITY.  Callers size the output with it.
 *   bounds       bounds[b] = min over the rows written of (w_0 + 0.0f, w_1 + 0.0f, w_2 + 0.0f), then the max of the same: the sum
 *                turns -0 into +0, so the result does not depend on the order of the reduction.  Nothing written: +inf x 3, -inf x 3.
 *   refresh_state   non-zero: every chosen map also gets state[r] = (w_0, w_1, w_2, state[r][3] as it was) for every r < n_points
 *                whose world coordinates are finite, whatever the filter and out_stride say, in the archive slot or in maps.state
 *                for the live map; legal in a count-only call.  This is the global landmark update.  Zero: no input is written.
 * status[b]: PRS_ERR_RANGE, with n_out[b] = n_total[b] = n_nonfinite[b] = 0 and nothing else of the sequence written (no row, no
 * bounds, no state): n_nodes[b] outside [1, node_stride]; cur_node[b] outside [0, n_nodes[b]); with include_live, the live n_points[b]
 * outside [0, capacity]; a used slot_of_node entry >= slot_stride; a used slot's n_points outside [0, capacity]; two used nodes that
 * name the same slot (its state rows would be refreshed twice).  "Used": of a node below n_nodes[b] that the live map does not
 * replace.  Otherwise PRS_ERR_CAPACITY as above, or PRS_OK.  A sequence never writes outside its rows.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, coords, desc, n_points, graph_X, n_nodes or
 * cur_node of the session, n_opt or inlier of maps, coords, desc, n_opt, inlier, n_points or slot_of_node of the archive, n_out,
 * n_total, n_nonfinite, status or the workspace unset; with refresh_state also state of maps and of the archive; desc, node, row,
 * n_opt and bounds of the output are optional); PRS_ERR_RANGE (batch, capacity or node_stride differ between the three structs or
 * are < 1, slot_stride < 1, out_stride < 0, or out_stride < 1 with xyz set); PRS_ERR_UNSUPPORTED (xyz, desc, coords, a state that is
 * written or the workspace not 16-byte aligned, graph_X not 8-byte aligned, another array not 4-byte aligned; batch * (slot_stride +
 * 1) * ceil(capacity / 256) beyond 2^24 - 1 workgroups, or batch workgroups of the scan's min(1024, node_stride rounded up to 64)
 * threads or of the bounds launch's min(1024, (slot_stride + 1) * ceil(capacity / 256) rounded up to 64) beyond the 2^32 - 1
 * work-items of one launch -- batch <= 2^22 - 1 where either has 1024 threads: prs_launch_fits --, or (slot_stride + 1) * capacity
 * beyond 2^31 - 1 rows).
 * A stable stream compaction spread over (sequence, map, chunk of 256 rows), so that one sequence of hundreds of maps fills the
 * device: count (a workgroup per chunk), scan (a workgroup per sequence: validation, node order, chunk bases), scatter (a workgroup
 * per chunk: ballots, wave totals in LDS, the scanned base) and, with bounds, a reduction per sequence.  Up to four plain launches
 * on the context's stream; no allocation, no synchronisation, no host read: graph-capturable.  No atomic decides a position or a
 * value: the output bytes depend neither on the batch around a sequence nor on the run.  Everything transient lives in the
 * caller's workspace, which two calls in flight must not share.
 * ============================================================================================== */
typedef struct {
  uint32_t min_n_opt;     /* keep landmarks optimised at least this often (0: all) */
  int32_t require_inlier; /* non-zero: keep only landmarks whose inlier flag is set */
  int32_t include_live;   /* non-zero: the current node's map is the live one */
  int32_t refresh_state;  /* non-zero: rewrite `state` of every chosen map from the graph */
} prs_world_map_params;

/* device pointers */
typedef struct {
  int32_t out_stride;     /* rows per sequence of the output arrays */
  int32_t reserved;
  float* xyz;             /* out [batch][out_stride][4], 16-byte aligned, or NULL = count only */
  uint8_t* desc;          /* out [batch][out_stride][32], 16-byte aligned (NULL allowed: not written) */
  int32_t* node;          /* out [batch][out_stride] graph node of the landmark's map (NULL allowed) */
  int32_t* row;           /* out [batch][out_stride] its row in that map (NULL allowed) */
  uint32_t* n_opt;        /* out [batch][out_stride] (NULL allowed) */
  int32_t* n_out;         /* out [batch] rows written */
  int32_t* n_total;       /* out [batch] rows that pass the filter, whatever out_stride is */
  int32_t* n_nonfinite;   /* out [batch] rows dropped because a world coordinate is not finite */
  float* bounds;          /* out [batch][6] min xyz, max xyz over the rows written (NULL allowed) */
  int32_t* status;        /* out [batch] */
  void* workspace;        /* prs_world_map_workspace_bytes(batch, slot_stride, capacity) bytes, 16-byte aligned */
} prs_world_map_batch;

/* bytes of workspace a call over `batch` sequences of an archive of slot_stride slots of `capacity` rows needs (0: a size below 1) */
PRS_API uint64_t prs_world_map_workspace_bytes(int32_t batch, int32_t slot_stride, int32_t capacity);
/* device pointers, asynchronous on the context's stream.  maps supplies the live map's n_opt, inlier and state; its coords, desc
 * and n_points are the session's */
PRS_API int prs_world_map_batch_run(prs_context* ctx, const prs_world_map_params* params, const prs_session_batch* session,
                                    const prs_merge_batch* maps, const prs_map_archive* archive, const prs_world_map_batch* out);
/* sizeof prs_world_map_params, prs_world_map_batch as the library was compiled (bindings check) */
PRS_API void prs_world_map_struct_sizes(uint64_t* sizes2);

/* ================================================================================================
 * World voxel filter: the rows of a world-frame landmark cloud that lie in one cubic voxel are fused into one row.  A split resets
 * the live map, so the next local map triangulates again what the previous one held, and every revisit adds another copy: the
 * world map's cloud holds one physical corner many times over.  This stage consumes the world map's output arrays in place (or any
 * cloud of the same layout) and hands out one row per voxel; the maps themselves and the archive keep their duplicates.
 *
 * BUILD-DEFINED: the reference writes no map, so the rule below is this build's.  tests/world_voxel_ref.py restates it in numpy and
 * the kernels equal that byte for byte.  All arithmetic is explicit two-operand float64 in the order written, -ffp-contract=off.
 * With s = (double) voxel_size, per sequence b:
 *
 *   rows         n = in_n[b]; the rows are i = 0 .. n - 1 and (x_0, x_1, x_2) = in_xyz[b][i][0..2].  A row with a coordinate that
 *                is not finite is dropped and counted in n_nonfinite[b].
 *   voxel        k_a = floor((double) x_a / s).  A row with some k_a outside [-2^20, 2^20) is dropped and counted in
 *                n_outside[b].  The voxel key is ((k_0 + 2^20) << 42) | ((k_1 + 2^20) << 21) | (k_2 + 2^20): below 2^63, so an
 *                all-ones word can mark an empty slot.  floor, not truncation: -1e-30 lies in voxel -1, and -0.0 in voxel 0.
 *   representative   of the rows of one voxel the one with the greatest n_opt, among equals the smallest i: as a packed key the
 *                minimum of ((uint64) ~n_opt << 32) | i, which does not depend on the order of evaluation.  in_n_opt == NULL: every
 *                row has n_opt 0.  count is the number of rows of the voxel.
 *   position     PRS_VOXEL_REPRESENTATIVE: the representative's four input floats, bit for bit.
 *                PRS_VOXEL_MEAN: per axis f_a = (double) x_a - k_a * s, q_a = (int64) rint((f_a / s) * 1073741824.0), S_a = the
 *                integer sum of q_a over the voxel's rows (exact, free of order, |S_a| < 2^62 for any in_stride),
 *                m_a = (float) ((k_a + ((double) S_a / (double) count) / 1073741824.0) * s); the output row is
 *                (m_0, m_1, m_2, w of the representative).
 *                Descriptors are never averaged: desc, node, row and n_opt always come from the representative, which is why one
 *                is chosen and not only a centroid computed.  Each of the four is written only when both its input and its output
 *                are set.
 *   order        voxels by their representative's i, ascending: the output is a subsequence of the input cloud and keeps its
 *                node-then-row order.  Voxel j < out_stride is written to xyz[b][j], index[b][j] (the representative's i),
 *                count[b][j] and the gathered arrays; rows from n_out[b] on are left untouched.  n_voxels[b] is the true number of
 *                voxels; n_voxels[b] > out_stride: status[b] = PRS_ERR_CAPACITY, n_out[b] = out_stride and those rows are valid.
 *   count only   xyz == NULL: n_voxels, n_nonfinite, n_outside and status are written, n_out[b] = 0, nothing else is touched.
 *   table        table_stride, a power of two >= 1, gives the slots of a sequence's hash table.  A sequence with more voxels than
 *                slots: status[b] = PRS_ERR_CAPACITY, n_out[b] = 0, n_voxels[b] = -1 (which tells it from truncation) and no row
 *                written; n_nonfinite and n_outside are still written.  The probing visits every slot, so an insertion fails only
 *                when the table is full of other keys, which happens exactly when the sequence has more voxels than slots: the
 *                outcome does not depend on the run.
 * status[b]: PRS_ERR_RANGE, with n_out[b] = n_voxels[b] = n_nonfinite[b] = n_outside[b] = 0 and nothing else of the sequence
 * written: in_n[b] outside [0, in_stride].  Otherwise PRS_ERR_CAPACITY as above, or PRS_OK.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, in_xyz, in_n, n_out, n_voxels,
 * n_nonfinite, n_outside, status or the workspace unset); PRS_ERR_RANGE (batch or in_stride < 1, table_stride not a power of two
 * >= 1, voxel_size not finite or <= 0, an unknown position, out_stride < 1 with xyz set); PRS_ERR_UNSUPPORTED (in_xyz, in_desc, xyz,
 * desc or the workspace not 16-byte aligned, another array not 4-byte aligned; batch * ceil(in_stride / 256) or batch *
 * ceil(table_stride / 256) beyond 2^24 - 1 workgroups, the 2^32 - 1 work-items of one launch: prs_launch_fits).
 * Five plain launches on the context's stream (four in a count-only call): clear the tables, insert (one thread per row: the key,
 * linear probing by 64-bit compare-and-swap, then an integer min on the rank, an add on the count and, MEAN only, on the three
 * sums), flag the representatives and count them per chunk of 256 rows, scan (a workgroup per sequence: validation, table overflow,
 * chunk bases) and scatter (ballots plus the scanned base).  No allocation, no synchronisation, no host read: graph-capturable.
 * Every atomic is an integer min, add or compare-and-swap whose result is free of order; none decides a position or an output
 * value.  WHICH slot a voxel lands in may differ from run to run, no output byte does.  Everything transient lives in the caller's
 * workspace, which two calls in flight must not share.
 * ============================================================================================== */
#define PRS_VOXEL_REPRESENTATIVE 0
#define PRS_VOXEL_MEAN 1
typedef struct {
  float voxel_size;     /* edge of a voxel in metres, finite and > 0 */
  int32_t position;     /* PRS_VOXEL_REPRESENTATIVE or PRS_VOXEL_MEAN */
  int32_t reserved[2];
} prs_world_voxel_params;

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t in_stride;         /* rows per sequence of the input arrays */
  const float* in_xyz;       /* in [batch][in_stride][4], 16-byte aligned (the world map's xyz) */
  const int32_t* in_n;       /* in [batch] rows of the sequence (the world map's n_out) */
  const uint32_t* in_n_opt;  /* in [batch][in_stride] (NULL allowed: every row has n_opt 0) */
  const uint8_t* in_desc;    /* in [batch][in_stride][32], 16-byte aligned (NULL allowed) */
  const int32_t* in_node;    /* in [batch][in_stride] (NULL allowed) */
  const int32_t* in_row;     /* in [batch][in_stride] (NULL allowed) */
  int32_t out_stride;        /* rows per sequence of the output arrays */
  int32_t table_stride;      /* slots per sequence of the hash table, a power of two */
  float* xyz;                /* out [batch][out_stride][4], 16-byte aligned, or NULL = count only */
  int32_t* index;            /* out [batch][out_stride] input row of the voxel's representative (NULL allowed) */
  int32_t* count;            /* out [batch][out_stride] rows fused into the voxel (NULL allowed) */
  uint8_t* desc;             /* out [batch][out_stride][32], 16-byte aligned (NULL allowed) */
  int32_t* node;             /* out [batch][out_stride] (NULL allowed) */
  int32_t* row;              /* out [batch][out_stride] (NULL allowed) */
  uint32_t* n_opt;           /* out [batch][out_stride] (NULL allowed) */
  int32_t* n_out;            /* out [batch] rows written */
  int32_t* n_voxels;         /* out [batch] voxels, whatever out_stride is; -1: more voxels than table_stride */
  int32_t* n_nonfinite;      /* out [batch] rows dropped because a coordinate is not finite */
  int32_t* n_outside;        /* out [batch] rows dropped because they lie outside the grid of 2^21 voxels per axis */
  int32_t* status;           /* out [batch] */
  void* workspace;           /* prs_world_voxel_workspace_bytes(batch, in_stride, table_stride) bytes, 16-byte aligned */
} prs_world_voxel_batch;

/* bytes of workspace a call needs: batch * (48 * table_stride + 16 + 4 * in_stride + 4 * ceil(in_stride / 256)), rounded up to 16
 * (0: a size below 1) */
PRS_API uint64_t prs_world_voxel_workspace_bytes(int32_t batch, int32_t in_stride, int32_t table_stride);
/* device pointers, asynchronous on the context's stream */
PRS_API int prs_world_voxel_batch_run(prs_context* ctx, const prs_world_voxel_params* params, const prs_world_voxel_batch* batch);
/* sizeof prs_world_voxel_params, prs_world_voxel_batch as the library was compiled (bindings check) */
PRS_API void prs_world_voxel_struct_sizes(uint64_t* sizes2);

/* ================================================================================================
 * Dispatch plans -- tests and tools only.  What a launch of the stereo matcher, the aligner, the brute-force matcher or the merger
 * WOULD run for a shape: the kernels by the names a kernel trace prints, grid, block, dynamic LDS bytes, the refusal if there is
 * one, and the layout facts the kernels' data-dependent paths hang on.  The library's launch functions consume the same plans.
 * Nothing here touches a device: the batch descriptors' pointers are only tested for being set, never followed, and a
 * prs_dispatch_env can be written by hand (a CU count, the knobs) or read from a live context.
 * ================================================================================================ */
typedef struct {
  int32_t cus;               /* compute units of the context's device (256 when the query failed) */
  int32_t fused_align;       /* PRS_FUSED_ALIGN */
  int32_t matcher_v3;        /* PRS_MATCHER_V3 */
  int32_t force_unstaged;    /* PRS_FORCE_UNSTAGED */
  int32_t no_lone_gn;        /* PRS_NO_LONE_GN */
  int32_t merge_fused;       /* PRS_MERGE_FUSED */
  int32_t bf_mfma;           /* PRS_BF_DENSE_* (prs_context_set_bruteforce_dense_phase) */
  int32_t stamps;            /* PRS_STAMPS */
  int32_t stamps_split;      /* PRS_STAMPS_SPLIT */
  int32_t bf_global_state;   /* PRS_BF_GLOBAL_STATE is set (read from the environment per launch) */
  int32_t bf_two_workgroups; /* PRS_BF_TWO_WORKGROUPS: -1 unset, 0, 1 (read from the environment per launch) */
  int32_t no_search_reuse;   /* PRS_NO_SEARCH_REUSE (appended with prs_context_get_search_reuse) */
} prs_dispatch_env;
PRS_API int prs_context_get_dispatch_env(const prs_context* ctx, prs_dispatch_env* env);

#define PRS_PLAN_MAX_LAUNCHES 4
#define PRS_PLAN_MAX_FACTS 48
typedef struct {
  const char* kernel; /* as a kernel trace prints it (static storage) */
  int32_t grid_x, grid_y, block;
  uint32_t lds_bytes; /* dynamic LDS */
} prs_plan_launch;
typedef struct {
  int32_t status;      /* PRS_OK or the refusal's status */
  const char* message; /* the refusal's message (static storage), NULL when there is none */
  int32_t n_launches;  /* 0: refused, or an empty batch */
  prs_plan_launch launch[PRS_PLAN_MAX_LAUNCHES];
  int32_t fact[PRS_PLAN_MAX_FACTS]; /* indexed by the family's PRS_PLAN_* enumerators; the rest is 0 */
} prs_dispatch_plan;

enum { PRS_DISPATCH_STEREO = 0, PRS_DISPATCH_ALIGN = 1, PRS_DISPATCH_BRUTEFORCE = 2, PRS_DISPATCH_MERGE = 3 };
/* stereo: V5 = 1 the second-generation kernel runs; V5_WHY = why it does not (0 it does, 1 stride, 2 knob, 3 cap, 4 lds, 5 best_lim);
 * CAP .. POOL_CAP: the v5 layout (set when v5 got that far); the first generation's staged / unstaged carve */
enum { PRS_PLAN_STEREO_V5, PRS_PLAN_STEREO_V5_WHY, PRS_PLAN_STEREO_CAP, PRS_PLAN_STEREO_OFF_POOL, PRS_PLAN_STEREO_POOL_CAP,
       PRS_PLAN_STEREO_V5_LDS, PRS_PLAN_STEREO_KPT, PRS_PLAN_STEREO_EPI, PRS_PLAN_STEREO_STAGE,
       PRS_PLAN_STEREO_STAGED_LDS, PRS_PLAN_STEREO_UNSTAGED_LDS, PRS_PLAN_STEREO_SORT_CAP, PRS_PLAN_STEREO_BEST_LIM };
enum { PRS_PLAN_ALIGN_MAX_FIXED, PRS_PLAN_ALIGN_CELL_SY, PRS_PLAN_ALIGN_CELL_SX, PRS_PLAN_ALIGN_CELL_NCY, PRS_PLAN_ALIGN_CELL_NCX,
       PRS_PLAN_ALIGN_LUT_CAP, PRS_PLAN_ALIGN_SPLIT, PRS_PLAN_ALIGN_SURV_SLOTS, PRS_PLAN_ALIGN_DB_BLOB, PRS_PLAN_ALIGN_LONE,
       PRS_PLAN_ALIGN_FIVE, PRS_PLAN_ALIGN_FAST, PRS_PLAN_ALIGN_PLAIN, PRS_PLAN_ALIGN_MPRIOR, PRS_PLAN_ALIGN_DEPTH,
       PRS_PLAN_ALIGN_OFF_U, PRS_PLAN_ALIGN_SEARCH_OFF_U };
enum { PRS_PLAN_BF_LIM, PRS_PLAN_BF_NW, PRS_PLAN_BF_CAP, PRS_PLAN_BF_GRID, PRS_PLAN_BF_CHUNKS, PRS_PLAN_BF_BM_FITS, PRS_PLAN_BF_LVL_CAP,
       PRS_PLAN_BF_FUSED_MATRIX, PRS_PLAN_BF_DUAL, PRS_PLAN_BF_MFMA, PRS_PLAN_BF_LDS, PRS_PLAN_BF_OFF_CNT_F, PRS_PLAN_BF_OFF_CNT_M,
       PRS_PLAN_BF_OFF_REG_F, PRS_PLAN_BF_OFF_REG_M, PRS_PLAN_BF_OFF_ACC, PRS_PLAN_BF_OFF_HIST, PRS_PLAN_BF_OFF_BM, PRS_PLAN_BF_OFF_LVL,
       PRS_PLAN_BF_OFF_MX };
enum { PRS_PLAN_MERGE_NBR, PRS_PLAN_MERGE_NBC, PRS_PLAN_MERGE_SPLIT, PRS_PLAN_MERGE_OFF_OWNER,
       PRS_PLAN_MERGE_OFF_FIRST, PRS_PLAN_MERGE_OFF_BEST, PRS_PLAN_MERGE_OFF_SEEN, PRS_PLAN_MERGE_OFF_SH, PRS_PLAN_MERGE_OFF_WAVE,
       PRS_PLAN_MERGE_OFF_POSE_CACHE, PRS_PLAN_MERGE_TAIL_CAPACITY };
PRS_API int prs_stereo_plan(const prs_stereo_params* params, const prs_stereo_batch* batch, const prs_dispatch_env* env, prs_dispatch_plan* plan);
PRS_API int prs_align_plan(const prs_pcf_params* finder, const prs_aligner_params* aligner, const prs_align_batch* batch, int32_t mode,
                           const prs_dispatch_env* env, prs_dispatch_plan* plan);
PRS_API int prs_bruteforce_plan(const prs_bruteforce_params* params, const prs_bruteforce_batch* batch, const prs_dispatch_env* env,
                                prs_dispatch_plan* plan);
PRS_API int prs_merge_plan(const prs_merger_params* params, const prs_merge_batch* batch, const prs_dispatch_env* env, prs_dispatch_plan* plan);
/* the index-th kernel of a family's variant tables (every kernel a plan of that family can name); NULL past the end */
PRS_API const char* prs_dispatch_kernel_name(int32_t family, int32_t index);
/* sizeof prs_dispatch_env, prs_dispatch_plan as the library was compiled (bindings check) */
PRS_API void prs_dispatch_struct_sizes(uint64_t* sizes2);

/* ================================================================================================
 * Trajectory evaluator: ATE, RPE and the KITTI metric of B trajectories against ground truth, on the device
 * stands where the reference's five benchmarks/benchmark_*.cpp feed every pose to a benchmark suite and fail on
 * isRegression(mean / std translation, mean / std rotation) (benchmark_kitti.cpp:17-20 and its four siblings).  It reads the layout
 * prs_session_unroll_batch writes, in place: one launch after the unroll gives one figure of merit per sequence without a host read.
 *
 * BUILD-DEFINED: the suite (srrg_benchmark) is not in the tree, so nothing below is the reference's own definition.  The metrics are
 * the published ones: the absolute trajectory error after a closed-form rigid alignment (Horn 1987 / Umeyama 1991 without scale) and
 * the fixed-delta relative pose error as TUM's evaluate_ate.py / evaluate_rpe.py state them (Sturm et al., IROS 2012), and the KITTI
 * odometry devkit's subsequence errors (evaluate_odometry.cpp: trajectoryDistances, lastFrameFromSegmentLength, calcSequenceErrors).
 * Ours, not theirs: the rotation angle by atan2 where both use acos; the rigid inverse [R^T | -R^T t] for every inverse; path_length
 * and the per-axis block, which exists so that the four Vector3f thresholds of the reference's benchmarks have a counterpart;
 * population standard deviations; the treatment of invalid rows.  tests/trajectory_ref.py restates all of it in numpy.
 *
 * All arithmetic is float64 on the float32 inputs.  P_k is the estimate's row k, G_k the ground truth's, n = min(n_frames[b],
 * frame_stride); a row counts when k < n and valid[b][k] != 0 (no valid array: every row).  t(X) is the translation, R(X) the rotation.
 *   alignment   NONE: S = I.  FIRST: S = G_f P_f^-1 at the first valid row f.  RIGID: S = [R | c_G - R c_P] with c_P, c_G the
 *               centroids of the valid rows' translations and R the proper rotation (det = +1) that minimises sum |t(G_k) - S t(P_k)|^2:
 *               both clouds are centred in float64, M = sum (t(P_k) - c_P)(t(G_k) - c_G)^T, and R is the rotation of the unit
 *               quaternion that is the eigenvector of the largest eigenvalue of Horn's symmetric 4x4 N(M) (cyclic Jacobi, 12 sweeps).
 *               A quaternion gives a proper rotation also where the unconstrained optimum is a reflection.  Collinear (or coincident)
 *               clouds are NOT detected: the largest eigenvalue is then repeated and R is one of the minimisers, whichever the
 *               iteration lands on.  Fewer than 3 valid rows under RIGID, or none under FIRST: result[b].status = PRS_ERR_RANGE,
 *               n_valid is written, n_rpe = n_kitti = 0, every metric is 0, S = I and frame_error[b][..] = -1.
 *   ATE         e_k = |t(G_k) - S t(P_k)| over the valid rows: rmse, mean, max.  frame_error[b][k] = (float) e_k, -1 for every other
 *               row k < frame_stride.
 *   path_length sum of |t(G_k) - t(G_k-1)| over the k for which rows k and k - 1 are both valid.
 *   RPE         for every k with k + rpe_delta < n and both rows valid (n_rpe of them): dG = G_k^-1 G_k+d, dP = P_k^-1 P_k+d,
 *               E = dG^-1 dP, with X^-1 Y = [Rx^T Ry | Rx^T (ty - tx)].  Translation error |t(E)|; rotation error theta =
 *               atan2(|v| / 2, (tr R(E) - 1) / 2) with v = (R21 - R12, R02 - R20, R10 - R01) (|v| = 2 sin theta; no acos, which
 *               loses half the digits at small angles): rmse, mean, max of each.
 *   axis block  over the same pairs, mean and population standard deviation of |t(E)_i| (metres) and of |theta v_i / |v|| in degrees
 *               (0 when |v| = 0), i = x, y, z: accumulated as running means and squared deviations (Welford) and merged pairwise
 *               (Chan), so that a deviation far below the mean keeps its digits.  Within about 1e-6 rad of a half turn v is the
 *               difference of nearly equal numbers and vanishes at the half turn itself: theta stays accurate there, the DIRECTION
 *               does not, and the rotation components of the axis block are then meaningless (0 at |v| = 0).
 *   KITTI       only when kitti_step > 0, n > 0 and every row k < n is valid; n_kitti = 0 and zeros otherwise.  dist[k] = sum of
 *               |t(G_j) - t(G_j-1)| for 0 < j <= k, kept in workspace[b] (a block prefix sum in a fixed order).  For first = 0,
 *               kitti_step, 2 kitti_step, ... < n and each length L: last = the first index i with dist[i] > dist[first] + L (the
 *               devkit's linear scan; found by bisection, the same index on a non-decreasing array); no such index: the pair is
 *               skipped.  E as in RPE between rows first and last, t_err = |t(E)| / L, r_err = theta / L.  kitti_t / kitti_r are the
 *               means over all subsequences (a ratio; rad / m), kitti_*_len[i] the same per length, kitti_n_len[i] their number.
 * status per sequence: PRS_ERR_RANGE for n_frames[b] < 0 (treated as the alignment failure above, n_valid = 0) and for the alignment
 * failures; PRS_OK otherwise.  A sequence never writes outside its rows of result, frame_error and workspace.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (params, batch, estimate, ground_truth, n_frames or
 * result unset, or workspace unset with kitti_step > 0); PRS_ERR_RANGE (batch or frame_stride < 1, rpe_delta < 1, kitti_step < 0,
 * n_lengths outside 0..8, a length that is not finite, not positive or not above the one before it, an unknown align);
 * PRS_ERR_UNSUPPORTED (estimate or ground_truth not 16-byte aligned, result or workspace not 8-byte aligned).
 * One launch, one 512-thread workgroup per sequence, no allocation, no synchronisation, no host read: graph-capturable.  Every sum is
 * a fixed-order reduction (per-thread strided partials, wave shuffles, a tree over the waves in LDS) and there are no floating-point
 * atomics: a sequence's result bytes depend neither on the batch around it nor on the run.  The translations of both clouds (24
 * bytes a row) are staged in LDS once for the centroid, covariance, residual and distance passes while frame_stride <= 6400, and a
 * copy of dist beside them for the subsequence search while frame_stride <= 4800; beyond, the passes read global memory (same
 * arithmetic, same bytes).
 * ============================================================================================== */
enum { PRS_TRAJ_ALIGN_NONE = 0, PRS_TRAJ_ALIGN_FIRST = 1, PRS_TRAJ_ALIGN_RIGID = 2 };

typedef struct {
  int32_t align;        /* PRS_TRAJ_ALIGN_*: how the estimate is brought into the ground truth's frame before ATE */
  int32_t rpe_delta;    /* frames between the two ends of a relative pose, >= 1 */
  int32_t kitti_step;   /* a subsequence starts every kitti_step rows (devkit: 10); 0 skips the KITTI block */
  int32_t n_lengths;    /* 0 .. 8 */
  float   lengths[8];   /* metres, ascending (devkit: 100 .. 800) */
} prs_trajectory_params;

typedef struct {
  int32_t status, n_valid, n_rpe, n_kitti;
  double  S[16];                                   /* estimate -> ground-truth frame, as applied (row-major 4x4) */
  double  path_length;                             /* of the ground truth, metres */
  double  ate_rmse, ate_mean, ate_max;             /* metres */
  double  rpe_t_rmse, rpe_t_mean, rpe_t_max;       /* metres */
  double  rpe_r_rmse, rpe_r_mean, rpe_r_max;       /* radians */
  double  axis_t_mean[3], axis_t_std[3];           /* metres; |component| of the relative translation error */
  double  axis_r_mean[3], axis_r_std[3];           /* degrees; |component| of the relative rotation error's rotation vector */
  double  kitti_t, kitti_r;                        /* mean of t_err / len (ratio) and r_err / len (rad / m) over all subsequences */
  double  kitti_t_len[8], kitti_r_len[8];          /* the same means per length */
  int32_t kitti_n_len[8];
} prs_trajectory_result;

/* device pointers */
typedef struct {
  int32_t batch, frame_stride;
  const float*   estimate;      /* [batch][frame_stride][16], the layout prs_session_unroll_batch writes */
  const float*   ground_truth;  /* same layout, row k belongs to estimate row k */
  const int32_t* n_frames;      /* [batch]; clamped to frame_stride as the unroll clamps it */
  const uint8_t* valid;         /* optional [batch][frame_stride]; 0 = row has no ground truth or no estimate */
  prs_trajectory_result* result;/* out [batch], 8-byte aligned */
  float*  frame_error;          /* optional out [batch][frame_stride]: ATE residual per row, -1 where not valid */
  double* workspace;            /* [batch][frame_stride], needed when kitti_step > 0 */
} prs_trajectory_batch;

/* asynchronous on the context's stream: one kernel launch */
/* Launch size: a launch beyond 2^32 - 1 work-items is PRS_ERR_UNSUPPORTED with nothing enqueued or written (prs_launch_fits): a workgroup of 512 threads a sequence, batch <= 2^23 - 1. */
PRS_API int prs_trajectory_eval_batch(prs_context* ctx, const prs_trajectory_params* params, const prs_trajectory_batch* batch);
/* sizeof prs_trajectory_params, prs_trajectory_result, prs_trajectory_batch as the library was compiled (bindings check) */
PRS_API void prs_trajectory_struct_sizes(uint64_t* sizes3);

/* ================================================================================================
 * Image rectifier: raw frames are undistorted and stereo-rectified on the device, in front of the feature extractors and the RGB-D
 * preprocessor, whose image arrays it writes in place (dst has the layout of prs_extract_batch.images and prs_depth_batch.depth).
 *
 * BUILD-DEFINED: the reference has no such stage.  Both of its converters stamp distortion_model = "undistorted" on whatever they
 * are given (apps/convert_stereo_to_srrg2.cpp:145, apps/convert_rgbd_to_srrg2.cpp:147) and its epipolar matcher runs with
 * epipolar_line_thickness_pixels 0 (euroc.conf:535-551), so it needs images that are row-aligned to the pixel; EuRoC and TUM frames
 * are not recorded that way.  The rule below is this build's; tests/rectify_ref.py restates it in numpy and the kernel equals the
 * float32 restatement byte for byte.  Every operation is a two-operand float32 operation in the order written (-ffp-contract=off,
 * correctly rounded division).  For the destination pixel (u, v) of image b with m = maps[map_of[b]] (map_of == NULL: maps[0]):
 *
 *   ray       x = (u - dst_cx) / dst_fx, y = (v - dst_cy) / dst_fy; with R row-major, taking source-camera coordinates to
 *             rectified-camera coordinates (OpenCV's R1 / R2), the ray in the source camera is R^T (x, y, 1):
 *             rx = (R[0] x + R[3] y) + R[6], ry = (R[1] x + R[4] y) + R[7], rz = (R[2] x + R[5] y) + R[8].
 *   distort   xn = rx / rz, yn = ry / rz, xx = xn xn, yy = yn yn, xy = xn yn, r2 = xx + yy,
 *             rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),
 *             xd = (xn rad + (2 p1) xy) + p2 (r2 + 2 xx), yd = (yn rad + p1 (r2 + 2 yy)) + (2 p2) xy
 *             (PRS_DISTORTION_RADTAN, the radial-tangential model of OpenCV; all five coefficients 0: a pinhole).
 *   project   us = src_fx xd + src_cx, vs = src_fy yd + src_cy.
 *   border    the pixel is `border` unless rz > 0, us > -1, us < src_cols, vs > -1 and vs < src_rows all hold.  NaN fails every
 *             comparison, and no float outside that range is ever converted to an integer.
 *   bilinear  (PRS_PIXEL_U8 only) x0 = floor(us), y0 = floor(vs), ax = us - x0, ay = vs - y0; taps a = (y0, x0), b = (y0, x0 + 1),
 *             c = (y0 + 1, x0), d = (y0 + 1, x0 + 1) as floats, a tap outside the source reads `border`;
 *             top = a + ax (b - a), bot = c + ax (d - c), val = top + ay (bot - top); the output is
 *             (uint8) min(max(floor(val + 0.5f), 0), 255).
 *   nearest   xi = floor(us + 0.5f), yi = floor(vs + 0.5f): the source element's bits unchanged, `border` when (yi, xi) lies
 *             outside.  The depth image's mode: interpolating depth across an edge invents surfaces.
 *   border value   params->border converted once on the host: U8 / U16 (uint) min(max(floor(border + 0.5f), 0), 255 / 65535), NaN
 *             gives 0; F32 keeps its bits.
 * n_border[b] (optional) is the number of destination pixels of image b that are `border` by the border rule (not those with only
 * some taps outside); the entry clears it on the stream and each workgroup adds its tile's count with one integer atomic.
 * status[b]: PRS_ERR_RANGE when map_of[b] lies outside [0, n_maps) or the map has a field that is not finite, a focal length
 * (src_fx, src_fy, dst_fx, dst_fy) that is 0 or an unknown model: every pixel of the image is then `border` and n_border[b] =
 * dst_rows * dst_cols; the other images are unaffected.  PRS_OK otherwise.  Bytes of dst between dst_cols elements and dst_pitch are
 * never written.
 * Call-level (return value, nothing enqueued, outputs untouched): PRS_ERR_NULL (params, batch, src, dst, maps or status unset);
 * PRS_ERR_UNSUPPORTED (an unknown pixel_type or interpolation, bilinear for other than PRS_PIXEL_U8, dst not 4-byte aligned, src not
 * aligned to its element, src and dst overlapping, a launch beyond 2^32 - 1 work-items, which is 2^24 - 1 workgroups of 256 threads: prs_launch_fits); PRS_ERR_RANGE (batch, n_maps or a size below 1,
 * a pitch below cols * element size or not a multiple of the element size, an image of 2^31 bytes or more).
 * One kernel launch behind one clear of n_border on the context's stream: no allocation, no synchronisation, no host read,
 * graph-capturable like prs_extract_features_batch.  The map costs about a hundred vector instructions and two divisions a pixel,
 * the pixels far less, so a workgroup owns one destination tile (16 rows of 64 pixels: four adjacent pixels per lane, one 4-byte
 * store per lane for 8-bit pixels) and a chunk of up to 16 consecutive images; it holds (source offset, ax, ay, tap validity) in
 * registers and recomputes them only when map_of[b] differs from the map it holds, so callers that keep one camera's images
 * together (ops.RectifyBatch: left block, right block) pay for the map once per chunk.  Any order is correct.  The chunk shrinks
 * while the grid would not fill the chip (PRS_RECTIFY_CHUNK = 1 .. 64 in the environment, read per launch, fixes it: tests and
 * tools).  For 8-bit bilinear the workgroup stages the tile's source footprint -- the box around the taps it holds, in whole
 * 16-byte pieces of the source rows -- in LDS per image and reads the taps from there, when src and src_pitch are multiples of 16
 * bytes and the box fits 8 KB; otherwise, and for nearest, the lanes fetch their taps from global memory (PRS_RECTIFY_VARIANT = 0
 * forces that: tools).  Staging reads a source row up to the next multiple of 16 bytes, which lies inside src_pitch: with src and
 * src_pitch multiples of 16 bytes the LAST row of src therefore has cols rounded up to 16 bytes that belong to the array (their
 * values reach no pixel); in every other case src ends at its last pixel, and dst always does (a lane's four-pixel store is issued
 * only when all four lie inside dst_cols).  There is no host-pointer variant and no C++ adapter in plugin/: the reference has no
 * class to mirror.
 * ============================================================================================== */
enum { PRS_DISTORTION_RADTAN = 0 };
enum { PRS_PIXEL_U8 = 0, PRS_PIXEL_U16 = 1, PRS_PIXEL_F32 = 2 };
enum { PRS_RECTIFY_BILINEAR = 0, PRS_RECTIFY_NEAREST = 1 };

/* one camera's map, an element of a device array; 96 bytes */
typedef struct {
  int32_t model;                           /* PRS_DISTORTION_RADTAN; the field is there for fisheye and rational models */
  int32_t reserved;
  float src_fx, src_fy, src_cx, src_cy;    /* the raw camera's matrix */
  float k1, k2, p1, p2, k3;                /* its distortion, in OpenCV's order */
  float R[9];                              /* row-major, source camera -> rectified camera (the identity: undistortion only) */
  float dst_fx, dst_fy, dst_cx, dst_cy;    /* the rectified camera's matrix */
} prs_rectify_map;

typedef struct {
  int32_t pixel_type;      /* PRS_PIXEL_* */
  int32_t interpolation;   /* PRS_RECTIFY_*; bilinear needs PRS_PIXEL_U8 */
  float border;            /* value of a pixel that has no source */
  int32_t reserved;
} prs_rectify_params;

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t src_rows, src_cols, src_pitch;   /* pitches in bytes, multiples of the element size */
  const void* src;                         /* [batch][src_rows][src_pitch]; ends at its last pixel, or, with src and src_pitch
                                              multiples of 16, at the last row's cols rounded up to 16 bytes (see above) */
  int32_t dst_rows, dst_cols, dst_pitch;   /* the destination's size may differ from the source's */
  void* dst;                               /* out [batch][dst_rows][dst_pitch], 4-byte aligned; must not overlap src */
  int32_t n_maps;
  const prs_rectify_map* maps;             /* [n_maps] */
  const int32_t* map_of;                   /* [batch], or NULL: every image uses maps[0] */
  int32_t* n_border;                       /* out [batch] border pixels of the image, or NULL */
  int32_t* status;                         /* out [batch] */
} prs_rectify_batch;

/* device pointers, asynchronous on the context's stream */
PRS_API int prs_rectify_batch_run(prs_context* ctx, const prs_rectify_params* params, const prs_rectify_batch* batch);
/* sizeof prs_rectify_map, prs_rectify_params, prs_rectify_batch as the library was compiled (bindings check) */
PRS_API void prs_rectify_struct_sizes(uint64_t* sizes3);

/* ================================================================================================
 * Dense RGB-D cloud: every sampled depth pixel of a sequence's chosen frames, placed in the world by the trajectory.  The depth
 * images are those of prs_depth_batch.depth or the rectifier's dst, the poses the array prs_session_unroll_batch writes, and the
 * output has the world map's layout, so prs_world_voxel_batch_run reads it in place (frame and pixel in the places of in_node and
 * in_row).
 *
 * BUILD-DEFINED: the unprojector of apps/example_unproject_rgbd.cpp lives in srrg2_core, outside the reference tree, so the rule
 * below is this build's, put together from the depth test and scaling of RawDataPreprocessorMonocularDepth::_readDepth
 * (raw_data_preprocessor_monocular_depth.cpp:156-180), the unprojection of the depth merger and the float32 se3_mul / se3_apply of
 * the other stages; the app's range_min 0.1, range_max 10 and its depth scale 1e-3 are the defaults of the Python layer.
 * tests/depth_cloud_ref.py restates it in numpy and the kernels equal that byte for byte.  All arithmetic is explicit two-operand
 * float32 in the order written, -ffp-contract=off, division correctly rounded.  Per sequence b:
 *
 *   frames       f = 0 .. n_images[b] - 1 in order.  k = frame_index[b][f], or f when frame_index is NULL.  A frame whose k lies
 *                outside [0, pose_stride), or whose pose[b][k] has an entry that is not finite among the twelve of its top three
 *                rows, gives no row and is counted in n_skipped[b].  Otherwise T = se3_mul(pose[b][k], sensor_in_robot):
 *                T[i][j] = (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j < 3 and
 *                T[i][3] = ((A[i][0] * B[0][3] + A[i][1] * B[1][3]) + A[i][2] * B[2][3]) + A[i][3].
 *   pixels       v = 0, step, 2 step, .. < rows and inside a row u = 0, step, .. < cols, in raster order.  raw is the depth element
 *                as a float (a 16-bit value converts exactly).  The pixel is kept iff raw > 0 (which drops NaN, -0, 0 and negative
 *                values) and, with d = depth_scaling_factor_to_meters * raw, d >= range_min && d <= range_max (which drops +inf).
 *   point        p = (((float) u - cx) / fx * d, ((float) v - cy) / fy * d, d);
 *                w_i = ((T[i][0] * p_0 + T[i][1] * p_1) + T[i][2] * p_2) + T[i][3].  The row is (w_0, w_1, w_2, i) with i = 0.0f
 *                when gray is NULL and (float) gray(v, u) * (1.0f / 255.0f) otherwise.
 *   order        image, then raster, behind the first n_base[b] rows of the output (0 when n_base is NULL), which are not touched:
 *                the world map's node-then-row order.  frame[b][j] = f and pixel[b][j] = v * cols + u of row j.
 *   counts       n_total[b] = n_base[b] + the kept pixels, whatever out_stride is (saturating at 2^31 - 1);
 *                n_out[b] = min(n_total[b], out_stride); n_total[b] > out_stride: status[b] = PRS_ERR_CAPACITY, the rows below
 *                out_stride are valid.  Rows from n_out[b] on are left untouched.  n_base may be the pointer n_out: a long
 *                sequence is fed in several calls, each appending behind the last.
 *   count only   xyz == NULL: n_total, n_skipped and status (never PRS_ERR_CAPACITY) are written, n_out[b] = n_base[b], nothing
 *                else is touched.
 * status[b]: PRS_ERR_RANGE when n_images[b] lies outside [0, frames] or n_base[b] outside [0, out_stride], with
 * n_total[b] = n_skipped[b] = 0, n_out[b] = n_base[b] clamped into [0, out_stride] and no row written.  Otherwise PRS_ERR_CAPACITY
 * as above, or PRS_OK.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, depth, n_images, pose, n_out, n_total,
 * n_skipped, status or the workspace unset); PRS_ERR_RANGE (batch, frames, rows, cols, pose_stride or step < 1; pitch below
 * cols elements or not a multiple of the element size, gray_pitch below cols with gray set; a parameter that is not finite --
 * sensor_in_robot included --, a scale <= 0, range_min < 0 or range_min > range_max; out_stride < 1 with xyz set);
 * PRS_ERR_UNSUPPORTED (an unknown depth_type; xyz or the workspace not 16-byte aligned, depth not aligned to its element, another
 * array but gray not 4-byte aligned; rows * cols or frames * ceil(rows / step) * ceil(cols / step) beyond 2^31 - 1; a launch, the scan's
 * included, beyond 2^32 - 1 work-items, which is 2^24 - 1 workgroups of 256 threads: prs_launch_fits).
 * Three plain launches on the context's stream (two in a count-only call): count (a workgroup per chunk of 1024 sampled pixels of
 * one image, four consecutive samples a lane, wave ballots), scan (a workgroup per sequence: validation, the skipped frames,
 * n_base, truncation, the chunk bases) and scatter (the same ballots order the chunk's rows in LDS, from where they go out behind
 * the scanned base, one 16-byte store a row and 4 KB in one piece a store instruction of the workgroup; T once per workgroup
 * through LDS; chunks that keep nothing, lie behind out_stride or belong to a refused sequence return before they read a pixel).  With step 1, cols a multiple of 4 and rows 8-byte (16-bit) or 16-byte (float) aligned a lane reads its four
 * depths in one load.  No atomic at all; no allocation, no synchronisation, no host read: graph-capturable.  Everything transient
 * lives in the caller's workspace, which two calls in flight must not share.  There is no host-pointer variant, no colour output
 * and no C++ adapter in plugin/.
 * ============================================================================================== */
typedef struct {
  int32_t depth_type;                    /* PRS_DEPTH_U16 or PRS_DEPTH_F32 */
  float depth_scaling_factor_to_meters;  /* finite and > 0 */
  float fx, fy, cx, cy;                  /* the depth camera's matrix */
  float range_min, range_max;            /* metres, finite, 0 <= range_min <= range_max */
  int32_t step;                          /* pixel stride in both directions, >= 1 */
  float sensor_in_robot[16];             /* row-major; the identity when the poses are the camera's */
  int32_t reserved[3];
} prs_depth_cloud_params;

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t frames;              /* images per sequence */
  int32_t rows, cols;
  int32_t pitch;               /* bytes, a multiple of the depth element's size */
  int32_t gray_pitch;          /* bytes */
  int32_t pose_stride;         /* poses per sequence */
  int32_t out_stride;          /* rows per sequence of the output arrays */
  const void* depth;           /* in [batch][frames][rows][pitch] */
  const uint8_t* gray;         /* in [batch][frames][rows][gray_pitch] (NULL allowed: intensity 0) */
  const int32_t* n_images;     /* in [batch] */
  const float* pose;           /* in [batch][pose_stride][16], what prs_session_unroll_batch writes */
  const int32_t* frame_index;  /* in [batch][frames] the pose of image f (NULL allowed: f) */
  const int32_t* n_base;       /* in [batch] rows already in the output (NULL allowed: 0; may be n_out) */
  float* xyz;                  /* out [batch][out_stride][4], 16-byte aligned, or NULL = count only */
  int32_t* frame;              /* out [batch][out_stride] the image of the row (NULL allowed) */
  int32_t* pixel;              /* out [batch][out_stride] v * cols + u of the row (NULL allowed) */
  int32_t* n_out;              /* out [batch] rows of the output, the first n_base[b] included */
  int32_t* n_total;            /* out [batch] n_base[b] + kept pixels, whatever out_stride is */
  int32_t* n_skipped;          /* out [batch] frames without a usable pose */
  int32_t* status;             /* out [batch] */
  void* workspace;             /* prs_depth_cloud_workspace_bytes(...) bytes, 16-byte aligned */
} prs_depth_cloud_batch;

/* bytes of workspace a call needs: 4 * batch * frames * ceil(ceil(rows / step) * ceil(cols / step) / 1024), rounded up to 16
 * (0: a size below 1, or sampled pixels beyond 2^31 - 1) */
PRS_API uint64_t prs_depth_cloud_workspace_bytes(int32_t batch, int32_t frames, int32_t rows, int32_t cols, int32_t step);
/* device pointers, asynchronous on the context's stream */
PRS_API int prs_depth_cloud_batch_run(prs_context* ctx, const prs_depth_cloud_params* params, const prs_depth_cloud_batch* batch);
/* sizeof prs_depth_cloud_params, prs_depth_cloud_batch as the library was compiled (bindings check) */
PRS_API void prs_depth_cloud_struct_sizes(uint64_t* sizes2);

/* ================================================================================================
 * Dense stereo: a rectified pair to a dense disparity and depth image, between the rectifier's dst (left block, then right block:
 * the two pointers are separate, so it is read in place) and prs_depth_cloud_batch.depth (PRS_DEPTH_F32, scale 1: a depth of 0 is
 * what that stage drops).
 *
 * BUILD-DEFINED: the reference has no dense matcher, so the rule below is this build's.  Every decision is integer arithmetic; the
 * only rounded operations are one float32 division and one addition a pixel (sub-pixel) and one division (depth), correctly rounded,
 * -ffp-contract=off.  tests/dense_stereo_ref.py restates it in numpy and the kernels equal that byte for byte.  I(y, x) is the
 * pixel at clamped coordinates, y into [0, rows - 1], x into [0, cols - 1]; so are all coordinates below.
 *
 *   census       c(y, x): a 62-bit word, one bit per offset dy = -3 .. 3, dx = -4 .. 4 but the centre, I(y + dy, x + dx) < I(y, x).
 *                Only Hamming distances of the words are used.  cL of the left image, cR of the right.
 *   raw cost     d = min_disparity + i, i = 0 .. n_disparities - 1.  C_L(y, x, d) = popcount(cL(y, x) ^ cR(y, max(x - d, 0))),
 *                C_R(y, x, d) = popcount(cR(y, x) ^ cL(y, min(x + d, cols - 1))).
 *   aggregation  A_L(v, u, d) = the sum over dy, dx in [-r, r] of C_L(clamp(v + dy), clamp(u + dx), d), r = aggregation_radius;
 *                A_R the same over C_R.  At most 62 * 15 * 15 = 13950.
 *   admissible   d for a left pixel u iff u - d >= 0, for a right pixel x iff x + d <= cols - 1.  Every minimum runs over
 *                admissible d only; a pixel without one is invalid.
 *   winner       d* = the admissible d of least A, the lowest on a tie; A0 its cost.  A2 = the least A over admissible d with
 *                |d - d*| >= 2, or none.
 *   uniqueness   left only, uniqueness_percent = q > 0: kept iff A2 is none or 100 * A0 < (100 - q) * A2 in integers (strict: a
 *                flat region is rejected).  q = 0 keeps everything.
 *   left-right   lr_max_diff >= 0 (-1 turns the right pass off): with xr = u - d* and dR(v, xr) the winner of A_R at the right
 *                pixel (no uniqueness test), kept iff the right pixel has a winner and |dR - d*| <= lr_max_diff.
 *   sub-pixel    when d* - 1 and d* + 1 are both in the disparity range and admissible and
 *                den = (A(d* - 1) + A(d* + 1)) - 2 * A0 > 0: delta = (float) (A(d* - 1) - A(d* + 1)) / (float) (2 * den);
 *                otherwise delta = 0.  s = (float) d* + delta.
 *   output       valid iff kept and s > 0.  disparity(v, u) = s and depth(v, u) = bf / s when valid, else 0.0f both; bf = focal
 *                length * baseline in pixel * metres.  n_valid[b][f] = the valid pixels of the image.  Pad columns are not touched.
 *   sequences    images f >= n_images[b] are not touched (n_images NULL: frames).  status[b] = PRS_ERR_RANGE when n_images[b]
 *                lies outside [0, frames], and nothing of that sequence is written; otherwise PRS_OK.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, left, right, status or the workspace
 * unset, or disparity and depth both unset); PRS_ERR_RANGE (n_disparities outside 1 .. 256, min_disparity < 0 or
 * min_disparity + n_disparities > 4096, aggregation_radius outside 0 .. 7, uniqueness_percent outside 0 .. 99, lr_max_diff outside
 * -1 .. 255, bf not finite or <= 0; batch, frames, rows or cols < 1, left_pitch or right_pitch < cols, out_pitch < 4 * cols or not a
 * multiple of 4); PRS_ERR_UNSUPPORTED (disparity, depth, n_images, n_valid or status not 4-byte aligned, the workspace not 16-byte;
 * batch * frames * rows * cols beyond 2^31 - 1; a launch beyond 2^32 - 1 work-items, which is 2^24 - 1 workgroups of 256 threads:
 * prs_launch_fits).
 * Four plain launches on the context's stream (three with lr_max_diff = -1): census (a workgroup per 64 x 16 tile of an image, the
 * tile and its halo in LDS once), match for the left and for the right reference and each radius (a workgroup owns 64 - 2 r columns of a band of 32
 * rows and walks down it: lane x of each of its four waves is column x of the tile with its halo, a wave takes every fourth pair
 * of disparities, two 16-bit sums to a word; the vertical sums live in LDS and get the entering row's costs added and the leaving
 * row's subtracted, both recomputed by 64-bit popcounts from two staged census rows; 2 r + 1 LDS reads give the box sum, a packed
 * (cost, i) minimum the winner; the cost volume is never stored) and finish (a workgroup 8 rows of an image: left-right check,
 * outputs, n_valid by wave ballots and one integer atomic add a workgroup).  No persistent workgroup and no spinning; no allocation, no synchronisation, no host read: graph-capturable.
 * Everything transient lives in the caller's workspace, which two calls in flight must not share.  Left out, with reserved words
 * in the parameters for them: a median or hole filling, other census windows, 16-bit images; semi-global path aggregation is a
 * stage of its own beside this one (prs_sgm_stereo_batch_run, below) and the speckle filter one behind it
 * (prs_speckle_batch_run, below).  There is no host-pointer variant and no
 * C++ adapter in plugin/.
 * ============================================================================================== */
typedef struct {
  int32_t n_disparities;       /* 1 .. 256 */
  int32_t min_disparity;       /* >= 0, min_disparity + n_disparities <= 4096 */
  int32_t aggregation_radius;  /* r, 0 .. 7: a (2 r + 1)^2 box */
  int32_t uniqueness_percent;  /* q, 0 .. 99; 0 = no test */
  int32_t lr_max_diff;         /* -1 .. 255; -1 = no right pass */
  float bf;                    /* focal length * baseline, pixel * metres, finite and > 0 */
  int32_t reserved[6];
} prs_dense_stereo_params;

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t frames;              /* pairs per sequence */
  int32_t rows, cols;
  int32_t left_pitch;          /* bytes */
  int32_t right_pitch;         /* bytes */
  int32_t out_pitch;           /* bytes of a row of disparity and of depth, a multiple of 4 */
  int32_t reserved0;
  const uint8_t* left;         /* in [batch][frames][rows][left_pitch] */
  const uint8_t* right;        /* in [batch][frames][rows][right_pitch] */
  const int32_t* n_images;     /* in [batch] (NULL allowed: frames) */
  float* disparity;            /* out [batch][frames][rows][out_pitch / 4] (NULL allowed when depth is set) */
  float* depth;                /* out [batch][frames][rows][out_pitch / 4] (NULL allowed when disparity is set) */
  int32_t* n_valid;            /* out [batch][frames] (NULL allowed) */
  int32_t* status;             /* out [batch] */
  void* workspace;             /* prs_dense_stereo_workspace_bytes(...) bytes, 16-byte aligned */
} prs_dense_stereo_batch;

/* bytes of workspace a call needs.  With P = batch * frames * rows * cols and up16(x) = x rounded up to a multiple of 16:
 * 3 * up16(8 P) (the two census images and the left pass's records) + up16(2 P) when lr_check != 0 (the right pass's winners).
 * n_disparities does not enter but through its range.  0: a size below 1, n_disparities outside 1 .. 256, or P beyond 2^31 - 1 */
PRS_API uint64_t prs_dense_stereo_workspace_bytes(int32_t batch, int32_t frames, int32_t rows, int32_t cols, int32_t n_disparities,
                                                  int32_t lr_check);
/* device pointers, asynchronous on the context's stream */
PRS_API int prs_dense_stereo_batch_run(prs_context* ctx, const prs_dense_stereo_params* params, const prs_dense_stereo_batch* batch);
/* sizeof prs_dense_stereo_params, prs_dense_stereo_batch as the library was compiled (bindings check) */
PRS_API void prs_dense_stereo_struct_sizes(uint64_t* sizes2);

/* ================================================================================================
 * Speckle filter: the small connected segments of a disparity or depth image are set to 0, in place, between
 * prs_dense_stereo_batch.disparity (with depth as the companion) or a 16-bit depth image (prs_depth_batch.depth, the rectifier's
 * dst) and prs_depth_cloud_batch.depth, which drops a depth of 0.
 *
 * BUILD-DEFINED: the reference has no dense images, so the rule below is this build's; it follows OpenCV's filterSpeckles (the
 * speckleWindowSize and speckleRange of StereoBM / StereoSGBM).  Every decision is exact: one float32 subtraction and comparison a
 * pair of neighbours, integers otherwise.  tests/speckle_ref.py restates it in numpy and the kernels equal that byte for byte.
 * Per image f < n_images[b] of sequence b, independently; x(v, u) is the element of PRS_PIXEL_F32 or PRS_PIXEL_U16 (the
 * rectifier's constants) at row v, column u < cols:
 *
 *   valid        x(v, u) > 0.  For a float that drops NaN, +0, -0 and negative values; +inf is valid.
 *   connected    two 4-neighbours (left / right, up / down) iff both are valid and fabsf((float) a - (float) b) <= max_diff: one
 *                float32 subtraction, exact for 16-bit values.  inf - inf is NaN, so two +inf neighbours are not connected.
 *                Components are the transitive closure: a ramp of steps of max_diff is one component whatever its ends differ
 *                by.  Pad elements behind cols and the neighbouring images are never neighbours.
 *   label        label(v, u) = the least raster index v * cols + u over the pixel's component; -1 for an invalid pixel.
 *   removal      a component of at most max_size pixels is removed: each of its pixels becomes 0 in image, and so does the
 *                element at the same (v, u) of companion when one is given (its own pixel type and pitch; whatever it held).
 *                No other element of either array is written, pad columns included.  max_size = 0 removes nothing.
 *   counts       n_kept[b][f] = the valid pixels left, n_removed[b][f] = the valid pixels set to 0.
 *   label output the labels as they stood before the removal, with their own pitch; pad columns are not written.
 *   sequences    images f >= n_images[b] are not touched (n_images NULL: frames).  status[b] = PRS_ERR_RANGE when n_images[b]
 *                lies outside [0, frames], and nothing of that sequence is written; otherwise PRS_OK.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, image, status or the workspace unset);
 * PRS_ERR_RANGE (batch, frames, rows or cols < 1; pitch -- or, with the array set, companion_pitch or label_pitch -- below cols
 * elements or not a multiple of the element size; max_diff not finite or < 0; max_size < 0); PRS_ERR_UNSUPPORTED (a pixel_type
 * -- or, with a companion, a companion_type -- that is unknown or PRS_PIXEL_U8; image or companion not aligned to its element,
 * n_images, label, n_kept, n_removed or status not 4-byte aligned, the workspace not 16-byte; companion or label overlapping
 * image; rows * cols or batch * frames * rows * cols beyond 2^31 - 1; a launch beyond 2^32 - 1 work-items, which is 2^24 - 1
 * workgroups of 256 threads: prs_launch_fits).
 * Four plain launches on the context's stream (three for an image of one tile): tile (a workgroup per 64 x 16 tile of an image:
 * the values in LDS, the runs of each row from one wave ballot, vertical unions in LDS, flattened, out goes the raster index of
 * the tile's root), seam (a thread per pixel pair across a tile border: the same union in global memory), flatten (a workgroup
 * 2048 pixels: each pixel's root, and the runs of equal roots in a wave add their lengths to the root's size until that is seen
 * above max_size) and apply (a workgroup 2048 pixels: the zeroes, label, and the counts by wave ballots and one integer atomic add
 * a workgroup and counter).  The atomics are integer min and add, so no output byte depends on the order they arrive in; every
 * loop strictly lowers an index or leaves; no workgroup waits for another.  No allocation, no synchronisation, no host read: graph-capturable.  Everything transient lives in
 * the caller's workspace, which two calls in flight must not share.  Left out: 8-connectivity, a median or hole filling, an
 * out-of-place destination (the caller clones what it wants to keep), a host-pointer variant and a C++ adapter in plugin/.
 * ============================================================================================== */
typedef struct {
  int32_t pixel_type;      /* of image: PRS_PIXEL_U16 or PRS_PIXEL_F32 */
  int32_t companion_type;  /* of companion, read when one is given: PRS_PIXEL_U16 or PRS_PIXEL_F32 */
  float max_diff;          /* finite and >= 0: neighbours this close are connected */
  int32_t max_size;        /* >= 0: components of at most this many pixels are removed; 0 removes nothing */
  int32_t reserved[4];
} prs_speckle_params;

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t frames;              /* images per sequence */
  int32_t rows, cols;
  int32_t pitch;               /* bytes of a row of image, a multiple of its element's size */
  int32_t companion_pitch;     /* bytes of a row of companion, a multiple of its element's size */
  int32_t label_pitch;         /* bytes of a row of label, a multiple of 4 */
  int32_t reserved0;
  void* image;                 /* in, out [batch][frames][rows][pitch] */
  void* companion;             /* in, out [batch][frames][rows][companion_pitch] (NULL allowed); must not overlap image */
  const int32_t* n_images;     /* in [batch] (NULL allowed: frames) */
  int32_t* label;              /* out [batch][frames][rows][label_pitch / 4] (NULL allowed); must not overlap image */
  int32_t* n_kept;             /* out [batch][frames] (NULL allowed) */
  int32_t* n_removed;          /* out [batch][frames] (NULL allowed) */
  int32_t* status;             /* out [batch] */
  void* workspace;             /* prs_speckle_workspace_bytes(...) bytes, 16-byte aligned */
} prs_speckle_batch;

/* bytes of workspace a call needs.  With P = batch * frames * rows * cols and up16(x) = x rounded up to a multiple of 16:
 * 2 * up16(4 P) (a parent and a size, int32, per pixel).  0: a size below 1, or rows * cols or P beyond 2^31 - 1 */
PRS_API uint64_t prs_speckle_workspace_bytes(int32_t batch, int32_t frames, int32_t rows, int32_t cols);
/* device pointers, asynchronous on the context's stream */
PRS_API int prs_speckle_batch_run(prs_context* ctx, const prs_speckle_params* params, const prs_speckle_batch* batch);
/* sizeof prs_speckle_params, prs_speckle_batch as the library was compiled (bindings check) */
PRS_API void prs_speckle_struct_sizes(uint64_t* sizes2);

/* ================================================================================================
 * Semi-global dense stereo: a rectified pair to a dense disparity and depth image by path-aggregated census costs (Hirschmueller's
 * SGM), a stage of its own beside prs_dense_stereo_batch_run with the same inputs, outputs and output layout, so the speckle
 * filter and the dense cloud read its images in place.  Where the box matcher rejects every pixel of an untextured surface (its
 * uniqueness test is strict on flat costs), the paths carry the disparity of the textured surroundings across it.
 *
 * BUILD-DEFINED: the reference has no dense matcher, so the rule below is this build's.  Every decision is integer arithmetic; the
 * only rounded operations are one float32 division and one addition a pixel (sub-pixel) and one division (depth), correctly rounded,
 * -ffp-contract=off.  tests/sgm_stereo_ref.py restates it in numpy and the kernels equal that byte for byte.  I(y, x) is the
 * pixel at clamped coordinates, y into [0, rows - 1], x into [0, cols - 1]; so are all coordinates of census and raw cost.
 *
 *   census       c(y, x): a 62-bit word, one bit per offset dy = -3 .. 3, dx = -4 .. 4 but the centre, I(y + dy, x + dx) < I(y, x).
 *                Only Hamming distances of the words are used.  cL of the left image, cR of the right.
 *   raw cost     d_i = min_disparity + i, i = 0 .. n_disparities - 1.  C(y, x, i) = popcount(cL(y, x) ^ cR(y, max(x - d_i, 0))),
 *                0 .. 62, defined for every i, admissible or not: admissibility enters only at the winner.
 *   paths        n_paths = 4: the directions of travel (dy, dx) = (0, +1) (0, -1) (+1, 0) (-1, 0); n_paths = 8 adds (+1, +1)
 *                (+1, -1) (-1, +1) (-1, -1).
 *   path cost    for a pixel p and its predecessor q = p - (dy, dx): L_r(p, i) = C(p, i) when q lies outside the image; otherwise,
 *                with m = min over k of L_r(q, k),
 *                L_r(p, i) = C(p, i) + min(L_r(q, i), L_r(q, i - 1) + P1, L_r(q, i + 1) + P1, m + P2) - m,
 *                terms with i - 1 or i + 1 outside 0 .. n_disparities - 1 left out.  P1 = p1 and P2 = p2 are constants (no
 *                intensity-adaptive P2), 0 <= P1 <= P2 <= 4095, so L_r <= 62 + P2 <= 4157: a path cost does not fit a byte.
 *   aggregate    S(p, i) = the sum of L_r(p, i) over the paths, at most 8 * 4157 = 33256: a uint16, below the "no cost" 0xffff.
 *   admissible   i for a left pixel u iff u - d_i >= 0.  Every minimum of the winner runs over admissible i only; a pixel without
 *                one is invalid.
 *   winner       i* = the admissible i of least S, the lowest on a tie; A0 its cost, d* = d_i*.  A2 = the least S over admissible i
 *                with |i - i*| >= 2, or none.
 *   uniqueness   uniqueness_percent = q > 0: kept iff A2 is none or 100 * A0 < (100 - q) * A2 in integers (strict: flat costs are
 *                rejected).  q = 0 keeps everything.
 *   left-right   lr_max_diff >= 0 (-1 turns the check off).  The right image's costs are read from the left volume, there is no
 *                second aggregation: S_R(y, x, i) = S(y, x + d_i, i), admissible iff x + d_i <= cols - 1; dR(y, x) = the admissible
 *                i of least S_R, the lowest on a tie (no uniqueness test).  With xr = u - d*: kept iff the right pixel xr has a
 *                winner and |dR(v, xr) - i*| <= lr_max_diff.
 *   sub-pixel    when i* - 1 and i* + 1 are both in the disparity range and admissible and
 *                den = (S(i* - 1) + S(i* + 1)) - 2 * A0 > 0: delta = (float) (S(i* - 1) - S(i* + 1)) / (float) (2 * den);
 *                otherwise delta = 0.  s = (float) d* + delta.
 *   output       valid iff kept and s > 0.  disparity(v, u) = s and depth(v, u) = bf / s when valid, else 0.0f both; bf = focal
 *                length * baseline in pixel * metres.  n_valid[b][f] = the valid pixels of the image.  Pad columns are not touched.
 *   sequences    images f >= n_images[b] are not touched (n_images NULL: frames).  status[b] = PRS_ERR_RANGE when n_images[b]
 *                lies outside [0, frames], and nothing of that sequence is written; otherwise PRS_OK.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, left, right, status or the workspace
 * unset, or disparity and depth both unset); PRS_ERR_RANGE (n_disparities outside 1 .. 256, min_disparity < 0 or
 * min_disparity + n_disparities > 4096, n_paths not 4 or 8, p1 < 0, p2 < p1 or p2 > 4095, uniqueness_percent outside 0 .. 99,
 * lr_max_diff outside -1 .. 255, bf not finite or <= 0; batch, frames, rows, cols or images_in_flight < 1, left_pitch or
 * right_pitch < cols, out_pitch < 4 * cols or not a multiple of 4); PRS_ERR_UNSUPPORTED (disparity, depth, n_images, n_valid or
 * status not 4-byte aligned, the workspace not 16-byte; batch * frames * rows * cols beyond 2^31 - 1; a launch of a chunk, of the
 * census or of the finish beyond 2^32 - 1 work-items, which is 2^24 - 1 workgroups of 256 threads: prs_launch_fits).
 * The S volume of one image is rows * cols * n_disparities uint16 (119 MB for a KITTI image at 128 disparities), so the call
 * works through the images b * frames + f in chunks of images_in_flight (a value above batch * frames counts as batch * frames)
 * and reuses one set of volumes for every chunk.  Plain launches on the context's stream, 2 + chunks * (n_paths + 2) of them
 * (n_paths + 1 with lr_max_diff = -1), a number the host knows: n_images is read on the device and the waves of skipped images leave at once.  census (dense stereo's
 * kernel, once for all images); per chunk one path launch a direction (a wave owns a line and walks it, its lanes hold the
 * disparities, up to four neighbouring ones a lane: a row for dy = 0; otherwise the line that starts at column x0 of the first row
 * and visits (y, (x0 + y * dx) mod cols), restarting with L = C where it wraps, which is the border rule above, so no wave needs
 * another wave's state; C is recomputed from the census words by 64-bit popcounts and never stored; m by a wave reduction, i - 1 and
 * i + 1 from the neighbouring register or lane; the first direction stores S, the later ones read, add and store: launches on one
 * stream are ordered, so there are no atomics), one winner launch (a wave a pixel at a time: the left winner with A2, uniqueness
 * and sub-pixel into dense stereo's records) and, with the left-right check, one right-winner launch (a workgroup 128 right pixels
 * of a row: the diagonals S(y, x + d_i, i) from the row's slice of the volume, staged in LDS 64 disparities at a time); finish
 * (dense stereo's kernel, once: left-right check, outputs, n_valid).  The volume is indexed with 64-bit offsets.  No persistent workgroup
 * and no spinning, no workgroup waits for another; no allocation, no synchronisation, no host read: graph-capturable.  Everything
 * transient lives in the caller's workspace, which two calls in flight must not share.  Left out: an intensity-adaptive P2, 16
 * paths, a median or hole filling, a host-pointer variant and a C++ adapter in plugin/.
 * ============================================================================================== */
typedef struct {
  int32_t n_disparities;       /* 1 .. 256 */
  int32_t min_disparity;       /* >= 0, min_disparity + n_disparities <= 4096 */
  int32_t p1;                  /* P1, the penalty of a step of one disparity along a path: 0 .. p2 */
  int32_t p2;                  /* P2, the penalty of any larger step: p1 .. 4095 */
  int32_t n_paths;             /* 4 or 8 */
  int32_t uniqueness_percent;  /* q, 0 .. 99; 0 = no test */
  int32_t lr_max_diff;         /* -1 .. 255; -1 = no left-right check */
  float bf;                    /* focal length * baseline, pixel * metres, finite and > 0 */
  int32_t reserved[4];
} prs_sgm_stereo_params;

/* device pointers: prs_dense_stereo_batch with images_in_flight in the place of reserved0 */
typedef struct {
  int32_t batch;
  int32_t frames;              /* pairs per sequence */
  int32_t rows, cols;
  int32_t left_pitch;          /* bytes */
  int32_t right_pitch;         /* bytes */
  int32_t out_pitch;           /* bytes of a row of disparity and of depth, a multiple of 4 */
  int32_t images_in_flight;    /* >= 1: the images whose S volumes the workspace holds at a time; the one the workspace was sized for */
  const uint8_t* left;         /* in [batch][frames][rows][left_pitch] */
  const uint8_t* right;        /* in [batch][frames][rows][right_pitch] */
  const int32_t* n_images;     /* in [batch] (NULL allowed: frames) */
  float* disparity;            /* out [batch][frames][rows][out_pitch / 4] (NULL allowed when depth is set) */
  float* depth;                /* out [batch][frames][rows][out_pitch / 4] (NULL allowed when disparity is set) */
  int32_t* n_valid;            /* out [batch][frames] (NULL allowed) */
  int32_t* status;             /* out [batch] */
  void* workspace;             /* prs_sgm_stereo_workspace_bytes(...) bytes, 16-byte aligned */
} prs_sgm_stereo_batch;

/* bytes of workspace a call needs.  With P = batch * frames * rows * cols, Q = min(images_in_flight, batch * frames) * rows * cols *
 * n_disparities and up16(x) = x rounded up to a multiple of 16: 3 * up16(8 P) (the two census images and the left winners' records)
 * + up16(2 P) when lr_check != 0 (the right winners) + up16(2 Q) (one uint16 volume S).  A call whose params have fewer disparities
 * than the workspace was sized for fits it.  0: a size or images_in_flight below 1, n_disparities outside 1 .. 256, or P beyond
 * 2^31 - 1 */
PRS_API uint64_t prs_sgm_stereo_workspace_bytes(int32_t batch, int32_t frames, int32_t rows, int32_t cols, int32_t n_disparities,
                                                int32_t lr_check, int32_t images_in_flight);
/* device pointers, asynchronous on the context's stream */
PRS_API int prs_sgm_stereo_batch_run(prs_context* ctx, const prs_sgm_stereo_params* params, const prs_sgm_stereo_batch* batch);
/* sizeof prs_sgm_stereo_params, prs_sgm_stereo_batch as the library was compiled (bindings check) */
PRS_API void prs_sgm_stereo_struct_sizes(uint64_t* sizes2);

/* ================================================================================================
 * Depth consistency filter: every depth pixel of a sequence's frames is cross-checked against the neighbouring frames through the
 * trajectory, between the speckle filter (or a depth sensor's images) and prs_depth_cloud_batch.depth, which reads out in place
 * and drops a depth of 0.  A pixel that too few neighbours see at the same place, or whose point lies in the free space too many
 * neighbours observed, is set to 0 (Merrell et al. 2007; the geometric consistency of multi-view stereo pipelines).
 *
 * BUILD-DEFINED: the reference has no dense images, so the rule below is this build's.  tests/depth_consistency_ref.py restates it
 * in numpy and the kernels equal that byte for byte.  All float32 arithmetic is explicit two-operand arithmetic in the order
 * written, -ffp-contract=off, division correctly rounded; the float64 part follows the same rules.  Per sequence b and image
 * f < n_images[b] (n_images NULL: frames):
 *
 *   pose         k = frame_index[b][f], or f when frame_index is NULL.  The frame is usable iff k lies in [0, pose_stride) and the
 *                twelve entries of the top three rows of pose[b][k] are finite: the dense cloud's test.  C_f = se3_mul(pose[b][k],
 *                sensor_in_robot) in float32 with the dense cloud's operation order; R_f its rotation, t_f its translation.
 *                An unusable frame gets an all-zero out image and zero support / violation, is counted in n_skipped[b], and its
 *                depth elements that pass the validity test are counted in n_removed[b][f] (n_kept[b][f] = 0).
 *   neighbours   the slots g = f - j * stride and g = f + j * stride, j = 1 .. window.  A slot exists iff 0 <= g < n_images[b] and
 *                frame g is usable.  Only counts are formed, so the order of the slots affects no output byte.
 *   relative     M = C_g^-1 C_f in float64 from the float32 C_f, C_g, then rounded to float32: dt = t_f - t_g per component;
 *                M[i][j] = (Rg[0][i] * Rf[0][j] + Rg[1][i] * Rf[1][j]) + Rg[2][i] * Rf[2][j];
 *                M[i][3] = (Rg[0][i] * dt[0] + Rg[1][i] * dt[1]) + Rg[2][i] * dt[2].  World poses reach kilometres (KITTI): the
 *                translations are subtracted first, in float64, so the baseline is exact to far below a millimetre.
 *   validity     of a depth element of any frame: raw is the element as a float; valid iff raw > 0 and, with
 *                d = depth_scaling_factor_to_meters * raw, d >= range_min && d <= range_max: the dense cloud's test.  An invalid own
 *                pixel gets out = 0, support = violation = 0 and is counted nowhere.
 *   vote         of slot g for the valid pixel (v, u) of f: p = (((float) u - cx) / fx * d, ((float) v - cy) / fy * d, d), the
 *                dense cloud's point; q_i = ((M[i][0] * p_0 + M[i][1] * p_1) + M[i][2] * p_2) + M[i][3].  No vote unless q_2 > 0.
 *                x = floorf((q_0 / q_2 * fx + cx) + 0.5f), y = floorf((q_1 / q_2 * fy + cy) + 0.5f).  No vote unless
 *                x >= 0 && x < (float) cols && y >= 0 && y < (float) rows, compared as floats before any conversion (NaN: no
 *                vote).  raw_g = the element of frame g at ((int) y, (int) x); no vote unless it is valid; d_g its scaled value.
 *                e = d_g - q_2, tol = max_rel_diff * q_2.  Support iff e >= -tol && e <= tol.  Violation iff e > tol: the neighbour
 *                sees past the point, which therefore lies in its free space.  e < -tol: occluded, no vote.
 *   decision     support(v, u) and violation(v, u) are the counts over the slots (uint8, at most 16).  The pixel is kept iff
 *                support >= min_support && violation <= max_violation.  out(v, u) = the input element, bit for bit and in the
 *                input's element type, when kept; 0 otherwise.  n_kept[b][f] / n_removed[b][f] = the valid pixels kept / zeroed.
 *   untouched    pad columns of out, support and violation; everything of the images f >= n_images[b].
 * status[b]: PRS_ERR_RANGE when n_images[b] lies outside [0, frames]: nothing of that sequence is written but status[b] and
 * n_skipped[b] = 0.  Otherwise PRS_OK.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, depth, pose, out, status or the
 * workspace unset); PRS_ERR_RANGE (batch, frames, rows, cols or pose_stride < 1; window outside 1 .. 8, stride < 1, min_support or
 * max_violation outside 0 .. 16, max_rel_diff not finite or < 0; a parameter that is not finite -- sensor_in_robot included --, a
 * scale <= 0, range_min < 0 or range_min > range_max; pitch or out_pitch below cols elements or not a multiple of the element
 * size, count_pitch below cols with support or violation set); PRS_ERR_UNSUPPORTED (an unknown depth_type; depth or out not
 * aligned to the element, the workspace not 16-byte, another array but support and violation not 4-byte; out, support or violation
 * overlapping depth -- neighbours are read while out is written --; rows or cols above 2^24; batch * frames * rows * cols beyond
 * 2^31 - 1; a launch, prepare's included, beyond 2^32 - 1 work-items, which is 2^24 - 1 workgroups of 256 threads: prs_launch_fits).
 * Two plain launches on the context's stream.  prepare (a workgroup per sequence): validation, the usable flags, n_skipped, status,
 * zeroes in n_kept / n_removed, and one 64-byte record per image and slot in the workspace -- M, the exists flag and, in slot 0,
 * the state of the image -- so the float64 work is done once per slot, never per pixel.  filter (a workgroup per 64 x 32 pixels of
 * one image, in eight steps of 64 x 4, a lane per pixel a step): the image's records through LDS, the slots in a uniform loop with
 * one gather each -- a step maps to a compact patch of the neighbour --, the counts by wave ballots and one integer atomic add a
 * workgroup and counter, so no byte depends on the order they arrive in.  The workgroups of an unusable frame write zeroes and read its depth only to count
 * n_removed; those of an image behind n_images or of a refused sequence return before they read a depth.  No allocation, no
 * synchronisation, no host read: graph-capturable.  Everything transient lives in the caller's workspace, which two calls in
 * flight must not share.  Left out: a fused (averaged) depth, a back-projection pixel-error test, per-frame intrinsics, bilinear
 * sampling of the neighbour, a companion image, any choice of key frames beyond window / stride / frame_index, a host-pointer
 * variant and a C++ adapter in plugin/.
 * ============================================================================================== */
typedef struct {
  int32_t depth_type;                    /* PRS_DEPTH_U16 or PRS_DEPTH_F32 */
  float depth_scaling_factor_to_meters;  /* finite and > 0 */
  float fx, fy, cx, cy;                  /* the depth camera's matrix, the same for every frame */
  float range_min, range_max;            /* metres, finite, 0 <= range_min <= range_max */
  int32_t window;                        /* neighbours on each side, 1 .. 8 */
  int32_t stride;                        /* frames between two neighbours, >= 1 */
  float max_rel_diff;                    /* finite and >= 0: |d_g - q_2| <= max_rel_diff * q_2 is support */
  int32_t min_support;                   /* 0 .. 16 */
  int32_t max_violation;                 /* 0 .. 16 */
  float sensor_in_robot[16];             /* row-major; the identity when the poses are the camera's */
  int32_t reserved[3];
} prs_depth_consistency_params;

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t frames;              /* images per sequence */
  int32_t rows, cols;
  int32_t pitch;               /* bytes of a row of depth, a multiple of the element's size */
  int32_t out_pitch;           /* bytes of a row of out, a multiple of the element's size */
  int32_t count_pitch;         /* bytes of a row of support and of violation */
  int32_t pose_stride;         /* poses per sequence */
  const void* depth;           /* in [batch][frames][rows][pitch] */
  const int32_t* n_images;     /* in [batch] (NULL allowed: frames) */
  const float* pose;           /* in [batch][pose_stride][16], what prs_session_unroll_batch writes */
  const int32_t* frame_index;  /* in [batch][frames] the pose of image f (NULL allowed: f) */
  void* out;                   /* out [batch][frames][rows][out_pitch], the element type of depth; must not overlap depth */
  uint8_t* support;            /* out [batch][frames][rows][count_pitch] (NULL allowed); must not overlap depth */
  uint8_t* violation;          /* out [batch][frames][rows][count_pitch] (NULL allowed); must not overlap depth */
  int32_t* n_kept;             /* out [batch][frames] (NULL allowed) */
  int32_t* n_removed;          /* out [batch][frames] (NULL allowed) */
  int32_t* n_skipped;          /* out [batch] frames without a usable pose (NULL allowed) */
  int32_t* status;             /* out [batch] */
  void* workspace;             /* prs_depth_consistency_workspace_bytes(...) bytes, 16-byte aligned */
} prs_depth_consistency_batch;

/* bytes of workspace a call needs: 64 * batch * frames * 2 * window (one record per image and slot: the twelve floats of M, the
 * exists flag, the image's state, two unused words), a multiple of 16.  0: a size below 1, window outside 1 .. 8, or
 * batch * frames beyond 2^31 - 1 */
PRS_API uint64_t prs_depth_consistency_workspace_bytes(int32_t batch, int32_t frames, int32_t window);
/* device pointers, asynchronous on the context's stream */
PRS_API int prs_depth_consistency_batch_run(prs_context* ctx, const prs_depth_consistency_params* params,
                                            const prs_depth_consistency_batch* batch);
/* sizeof prs_depth_consistency_params, prs_depth_consistency_batch as the library was compiled (bindings check) */
PRS_API void prs_depth_consistency_struct_sizes(uint64_t* sizes2);

#ifdef __cplusplus
}
#endif
#endif
