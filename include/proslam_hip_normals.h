/* proslam_hip_normals.h -- surface normals of depth images on the device (gfx950): the second public header of libproslam_hip.so.
 *
 * include/proslam_hip.h is pinned to the layout of PRS_ABI_VERSION 104; what this header declares joins it, as it stands here, at
 * the next layout bump, and this file then only includes the main header.  Until then: the entry points below are exported from
 * the same library, use PRS_API, the status codes, prs_context and PRS_DEPTH_U16 / PRS_DEPTH_F32 of the main header, and have
 * their own size query (prs_depth_normals_struct_sizes) in the place of prs_abi_check.  Both structs end in reserved words: memset
 * them to 0 before filling them in.
 */
#ifndef PROSLAM_HIP_NORMALS_H
#define PROSLAM_HIP_NORMALS_H

#include "proslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ================================================================================================
 * Depth normals: depth images to oriented surface normals, one (n0, n1, n2, w) a pixel in the camera frame, and optionally one
 * world-frame normal per row of the dense cloud prs_depth_cloud_batch_run made of the same images (its frame, pixel and n_out are
 * read in place), which prs_world_voxel_batch_run's index then carries to the fused cloud.  The depth images are those of
 * prs_depth_cloud_batch.depth: the sensor's, the dense or semi-global matcher's, or the consistency filter's out.
 *
 * BUILD-DEFINED, like the other dense stages: the reference has no dense stage.  The rule is the cross-product normal of an
 * organised cloud (KinectFusion; PCL's IntegralImageNormalEstimation) with a depth-edge gate.  tests/depth_normals_ref.py restates
 * it in numpy and the kernels equal that byte for byte.  All arithmetic is explicit two-operand float32 in the order written,
 * -ffp-contract=off, division and sqrtf correctly rounded, denormals kept (the code object's float mode; numpy does the same).
 * Per served image (b, f), f < n_images[b] (frames when n_images is NULL), and pixel (v, u):
 *
 *   valid        the dense cloud's test: raw is the depth element as a float; valid iff raw > 0 (which drops NaN, -0, 0 and
 *                negative values) and, with d = depth_scaling_factor_to_meters * raw, d >= range_min && d <= range_max.
 *   point        p = (((float) u - cx) / fx * d, ((float) v - cy) / fy * d, d), the cloud's.
 *   usable       a neighbour q of the centre c is usable iff it lies inside the image, is valid and
 *                fabsf(d_q - d_c) <= max_rel_diff * d_c.
 *   tangents     L = (v, u - radius), R = (v, u + radius), U = (v - radius, u), D = (v + radius, u).  tx: L and R usable:
 *                p(R) - p(L); R only: p(R) - p(c); L only: p(c) - p(L); neither: no normal.  ty: the same with D in R's place
 *                and U in L's.  Subtraction is component-wise.  w = the number of usable neighbours, 2 .. 4, as a float.
 *   raw normal   m0 = ty1 * tx2 - ty2 * tx1, m1 = ty2 * tx0 - ty0 * tx2, m2 = ty0 * tx1 - ty1 * tx0,
 *                len2 = (m0 * m0 + m1 * m1) + m2 * m2; no normal unless len2 > 0 && len2 <= FLT_MAX; n_i = m_i / sqrtf(len2);
 *                dot = (n0 * p0 + n1 * p1) + n2 * p2 with p = p(c); dot > 0: every n_i is negated.  The normal faces the camera.
 *   smoothing    smooth = s > 0: a pixel that has a raw normal sums the raw normals of its (2 s + 1)^2 window, in raster order
 *                (dv outer, du inner, the centre in its own place), a_i = a_i + n_i from a_i = 0.0f, over the window pixels that
 *                lie inside the image, have a raw normal and are usable against the centre's depth (the gate above).  With
 *                len2 = (a0 * a0 + a1 * a1) + a2 * a2 the same test and n_i = a_i / sqrtf(len2); the test failing: no normal.
 *                No second orientation step; w stays the centre's.  A pixel without a raw normal of its own gets none.
 *   output       normal[b][f][v][u] = (n0, n1, n2, w), and (0, 0, 0, 0) where there is no normal.  Every pixel of every served
 *                image is written; the images from n_images[b] on and refused sequences are not touched.
 *                n_normal[b][f] (optional) = the pixels of the image with w > 0 (integer adds: the same whatever their order).
 *   cloud rows   optional; row_frame, row_pixel, row_n, row_normal, n_bad_rows and pose are set together or row_frame, row_pixel,
 *                row_n, row_normal and n_bad_rows are all NULL (pose, frame_index and row_base are then not read).  Rows j in
 *                [row_base[b], min(row_n[b], row_stride)) are written, row_base NULL meaning 0; the rows below row_base[b] and
 *                from row_n[b] on are not touched, which mirrors the cloud's n_base append.  f = row_frame[b][j],
 *                q = row_pixel[b][j], k = frame_index[b][f] or f when frame_index is NULL.  The row is (0, 0, 0, 0) and counted
 *                in n_bad_rows[b] when f lies outside [0, n_images[b]), q outside [0, rows * cols), k outside [0, pose_stride)
 *                or one of the twelve top-row entries of pose[b][k] is not finite.  Otherwise, with (n0, n1, n2, w) =
 *                normal[b][f][q] and T = se3_mul(pose[b][k], sensor_in_robot) as in the dense cloud,
 *                wn_i = (T[i][0] * n0 + T[i][1] * n1) + T[i][2] * n2 and the row is (wn0, wn1, wn2, w), not renormalised.
 *                n_bad_rows[b] is written by every call with rows (0 when none is bad).
 * status[b]: PRS_ERR_RANGE when n_images[b] lies outside [0, frames] or, with rows, row_base[b] or row_n[b] lies outside
 * [0, row_stride] or row_base[b] > row_n[b]; nothing else of that sequence is written.  Otherwise PRS_OK.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, depth, normal or status unset, or the
 * row pointers set only in part); PRS_ERR_RANGE (batch, frames, rows or cols < 1, with rows pose_stride or row_stride < 1; pitch
 * below cols elements or not a multiple of the element size; radius outside [1, 8] or smooth outside [0, 3]; a parameter that is
 * not finite -- sensor_in_robot included --, a scale <= 0, range_min < 0 or range_min > range_max, max_rel_diff < 0);
 * PRS_ERR_UNSUPPORTED (an unknown depth_type; normal or row_normal not 16-byte aligned, depth not aligned to its element,
 * another array not 4-byte aligned; rows * cols, batch * frames or their product beyond 2^31 - 1; a launch beyond 2^32 - 1
 * work-items, which is 2^24 - 1 workgroups of 256 threads: prs_launch_fits).
 * Two plain launches on the context's stream, three with rows: head (a thread an image: status, and 0 into n_normal), tiles (a
 * workgroup per 64 x 16 tile of one image: the tile's depths in metres with a halo of radius + smooth in LDS, NaN for an invalid
 * pixel or one outside the image, so that one comparison is the whole gate; the raw normals of the tile and a halo of smooth in
 * LDS when smooth > 0; one 16-byte store a pixel, consecutive lanes on consecutive pixels; wave ballots and one integer atomic add
 * a workgroup for n_normal) and rows (a workgroup per 256 rows of a sequence: one 16-byte load and one 16-byte store a row).  All
 * index arithmetic into normal is 64-bit: the array reaches 32 GiB within 2^31 - 1 pixels.  No allocation, no synchronisation, no
 * host read, no workspace: graph-capturable.  Left out: PCA / plane-fit normals, curvature, a bilateral depth pre-filter, a
 * host-pointer variant and a C++ adapter in plugin/.
 * ============================================================================================== */
typedef struct {
  int32_t depth_type;                    /* PRS_DEPTH_U16 or PRS_DEPTH_F32 */
  float depth_scaling_factor_to_meters;  /* finite and > 0 */
  float fx, fy, cx, cy;                  /* the depth camera's matrix */
  float range_min, range_max;            /* metres, finite, 0 <= range_min <= range_max */
  int32_t radius;                        /* pixels from the centre to L, R, U and D, 1 .. 8 */
  int32_t smooth;                        /* half-width of the smoothing window, 0 (none) .. 3 */
  float max_rel_diff;                    /* the depth-edge gate, relative to the centre's depth; finite, >= 0 */
  float sensor_in_robot[16];             /* row-major; the identity when the poses are the camera's */
  int32_t reserved[5];
} prs_depth_normals_params;

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t frames;              /* images per sequence */
  int32_t rows, cols;
  int32_t pitch;               /* bytes, a multiple of the depth element's size */
  int32_t pose_stride;         /* poses per sequence (read with rows) */
  int32_t row_stride;          /* cloud rows per sequence (read with rows) */
  int32_t reserved0;
  const void* depth;           /* in [batch][frames][rows][pitch] */
  const int32_t* n_images;     /* in [batch] (NULL allowed: frames) */
  const float* pose;           /* in [batch][pose_stride][16], what prs_session_unroll_batch writes (with rows) */
  const int32_t* frame_index;  /* in [batch][frames] the pose of image f (NULL allowed: f) */
  const int32_t* row_frame;    /* in [batch][row_stride] prs_depth_cloud_batch.frame */
  const int32_t* row_pixel;    /* in [batch][row_stride] prs_depth_cloud_batch.pixel */
  const int32_t* row_n;        /* in [batch] prs_depth_cloud_batch.n_out */
  const int32_t* row_base;     /* in [batch] rows that are left as they are (NULL allowed: 0) */
  float* normal;               /* out [batch][frames][rows][cols][4], 16-byte aligned */
  int32_t* n_normal;           /* out [batch][frames] pixels with a normal (NULL allowed) */
  float* row_normal;           /* out [batch][row_stride][4], 16-byte aligned */
  int32_t* n_bad_rows;         /* out [batch] */
  int32_t* status;             /* out [batch] */
  void* reserved[3];
} prs_depth_normals_batch;

/* device pointers, asynchronous on the context's stream */
PRS_API int prs_depth_normals_batch_run(prs_context* ctx, const prs_depth_normals_params* params, const prs_depth_normals_batch* batch);
/* sizeof prs_depth_normals_params, prs_depth_normals_batch as the library was compiled (bindings check) */
PRS_API void prs_depth_normals_struct_sizes(uint64_t* sizes2);

#ifdef __cplusplus
}
#endif

#endif /* PROSLAM_HIP_NORMALS_H */
