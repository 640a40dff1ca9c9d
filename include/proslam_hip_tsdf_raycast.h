/* proslam_hip_tsdf_raycast.h -- a TSDF volume rendered into depth and normal images on the device (gfx950): the fourth public
 * header of libproslam_hip.so.
 *
 * include/proslam_hip.h is pinned to the layout of PRS_ABI_VERSION 104; what this header declares joins it, as it stands here, at
 * the next layout bump, and this file then only includes the main header.  Until then: the entry points below are exported from
 * the same library, use PRS_API, the status codes and prs_context of the main header, and have their own size query
 * (prs_tsdf_raycast_struct_sizes) in the place of prs_abi_check.  Every struct ends in reserved words: memset it to 0 before
 * filling it in.
 */
#ifndef PROSLAM_HIP_TSDF_RAYCAST_H
#define PROSLAM_HIP_TSDF_RAYCAST_H

#include "proslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ================================================================================================
 * TSDF raycast: the volume prs_tsdf_integrate_batch_run fuses (include/proslam_hip_tsdf.h: (tsdf, weight) a voxel, tsdf in units of
 * the truncation, positive in front of the surface, weight 0 = never observed), rendered from any pose into a float32 depth image
 * in metres and the model's own normal per pixel (Curless and Levoy 1996; KinectFusion's surface prediction).  The depth image is a
 * PRS_DEPTH_F32 image at scale 1 that the dense cloud, the depth normals, the consistency filter and the integrator read in place.
 *
 * BUILD-DEFINED, like the other dense stages: the reference has no dense stage.  tests/tsdf_raycast_ref.py restates the rule in
 * numpy and the kernels equal that byte for byte.  All arithmetic is explicit two-operand float32 in the order written,
 * -ffp-contract=off, division and sqrtf correctly rounded, denormals kept; se3_mul is that of csrc/prs_se3.h.
 *
 * ---- prs_tsdf_raycast_batch_run: depth, normal (out) <- volume (in) ----
 * Per sequence b, view r < n_views[b] (views when n_views is NULL) and pixel (v, u), v < rows, u < cols, with
 * (o0, o1, o2) = origin[b] the world position of the corner of voxel (0, 0, 0) and (n0, n1, n2) = (nx, ny, nz):
 *   view     k = view_index[b][r], or r when view_index is NULL.  The view is skipped, as the integrator skips a frame, when k lies
 *            outside [0, pose_stride) or one of the twelve top-row entries of pose[b][k] is not finite: it is counted in
 *            n_skipped[b], its depth and normal are written as 0 and its n_hit is 0.  Otherwise
 *            T = se3_mul(pose[b][k], sensor_in_robot) and c_a = T[a][3], the camera's centre.
 *   ray      dc = (((float) u - cx) / fx, ((float) v - cy) / fy, 1.0f), dw_a = (T[a][0] * dc0 + T[a][1] * dc1) + T[a][2] * dc2:
 *            the ray parameter l is the z depth of the point c + l * dw.
 *   slab     per axis a: lo_a = o_a + 0.5f * voxel_size, hi_a = o_a + ((float) n_a - 0.5f) * voxel_size, the box of the voxel
 *            centres.  When dw_a == 0: the ray misses when c_a < lo_a || c_a > hi_a, otherwise the axis does not bound it.  When
 *            dw_a != 0: t1 = (lo_a - c_a) / dw_a, t2 = (hi_a - c_a) / dw_a, near = t2 < t1 ? t2 : t1, far = t2 < t1 ? t1 : t2.
 *            l_in starts at range_min and is replaced by every near with near > l_in, l_out starts at range_max and is replaced
 *            by every far with far < l_out, the axes in the order 0, 1, 2.  The ray is marched iff it did not miss and
 *            l_in <= l_out.
 *   samples  l_k = l_in + (float) k * step for k = 0, 1, ... while l_k <= l_out and k < n, with q = (l_out - l_in) / step and
 *            n = (int) (q < 1048576.0f ? q : 1048576.0f) + 2 when q >= 0 and n = 0 otherwise (a NaN gives no sample).  n is the
 *            trip count the kernel fixes before its loop; under a pose that is a rigid transform it ends no ray early, because
 *            the call refuses a volume whose diagonal holds more than 1048576 steps (below).
 *            g_a = ((c_a + l_k * dw_a) - o_a) / voxel_size - 0.5f, i_a = floorf(g_a).  The sample is VALID iff every g_a is finite,
 *            every i_a >= 0.0f && i_a <= (float) (n_a - 2) && (int) i_a <= n_a - 2 (the last says nothing new up to 2^24 voxels
 *            along an axis, where the float is exact), and the eight voxels (i0 + dx, i1 + dy, i2 + dz), dx, dy, dz in {0, 1},
 *            all have w >= min_weight.  Its value s(g) is the trilinear interpolation of their tsdf with f_a = g_a - i_a and
 *            lerp(p, q, f) = p + f * (q - p): along x first for the four pairs (dy, dz), then along y for dz = 0 and for dz = 1,
 *            then along z.
 *   hit      the first valid sample with value t <= 0.0f ends the ray.  It is a hit iff k >= 1, sample k - 1 of the same ray is
 *            valid and its value tp > 0.0f; then l* = l_(k-1) + step * (tp / (tp - t)).  Otherwise the ray starts behind a
 *            surface or in unobserved space: no hit.  depth = l* iff l* >= range_min && l* <= range_max, otherwise 0; a pixel
 *            without a hit is 0.
 *   normal   at a pixel with depth > 0, with g* the grid coordinate g at l*: per axis m_a = s(g* + e_a) - s(g* - e_a), the sample
 *            rule above one voxel either way along a; len2 = (m0 * m0 + m1 * m1) + m2 * m2.  With all six samples valid and
 *            len2 > 0 && len2 <= FLT_MAX: q_a = m_a / sqrtf(len2) and the row is, in the camera's frame,
 *            ((T[0][i] * q0 + T[1][i] * q1) + T[2][i] * q2) for i = 0, 1, 2, and 1.0f.  Otherwise, and at a pixel with depth 0,
 *            the row is (0, 0, 0, 0).  The normal is the gradient towards observed free space; it is not re-oriented.
 *   counts   n_hit[b][r] (optional) = the pixels with depth > 0 (integer adds: the same whatever their order).  The views from
 *            n_views[b] on are not touched: neither depth, normal nor n_hit.  The pitch padding of depth is never written.
 * status[b]: PRS_ERR_RANGE when n_views[b] lies outside [0, views]; nothing of that sequence is then written but
 * n_skipped[b] = 0.  Otherwise PRS_OK.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, origin, volume, pose, depth, n_skipped,
 * status or workspace unset); PRS_ERR_RANGE (batch, views, rows, cols, pose_stride, nx, ny or nz < 1; pitch below 4 * cols or not
 * a multiple of 4; a parameter that is not finite, sensor_in_robot included; range_min < 0 or range_min > range_max;
 * voxel_size <= 0; step <= 0; ((float) nx + (float) ny + (float) nz) * voxel_size / step > 1048576.0f, which bounds the step count
 * of every ray before its loop starts); PRS_ERR_UNSUPPORTED (volume, normal or workspace not 16-byte aligned, another array not
 * 4-byte aligned; nx * ny * nz beyond (2^31 - 1) / 3, rows * cols or batch * views beyond 2^31 - 1; a launch beyond 2^32 - 1
 * work-items, which is 2^24 - 1 workgroups of 256 threads: prs_launch_fits).
 * Two plain launches on the context's stream.  head (a workgroup a sequence, a thread a view): status, n_skipped, 0 into n_hit,
 * and T with a served flag for every view into the workspace.  rays (a workgroup of 256 threads per tile of 16 x 16 pixels of one
 * view, a wave per 8 x 8 pixels of it, so that the 64 rays of a wave walk through neighbouring voxels and their gathers share
 * cache lines): T is a wave-uniform read, a voxel's (tsdf, w) one 8-byte load and the two corners along x 16 contiguous bytes; the
 * loop's trip count is fixed before the loop and the loop is left when a ballot shows no live lane; n_hit costs a ballot count a
 * wave and one integer atomic add a workgroup; a pixel is one 4-byte and one 16-byte store.  Indexing into volume, depth and
 * normal is 64-bit.  No float atomic, no allocation, no synchronisation, no host read: graph-capturable.
 *
 * Left out: empty-space skipping and adaptive steps; a vertex image; colour; ray-length rather than z parameterisation; a
 * host-pointer variant and a C++ adapter in plugin/.  A surface thinner than `step` can be stepped over.
 * ============================================================================================== */
typedef struct {
  float fx, fy, cx, cy;          /* the rendered camera's matrix */
  float range_min, range_max;    /* metres of z depth, finite, 0 <= range_min <= range_max */
  float sensor_in_robot[16];     /* row-major; the identity when the poses are the camera's */
  float voxel_size;              /* metres, finite, > 0: the volume's */
  float min_weight;              /* finite: a voxel below it counts as unobserved */
  float step;                    /* metres along z between two samples, finite, > 0 */
  int32_t reserved[3];
} prs_tsdf_raycast_params;

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t views;               /* images per sequence */
  int32_t rows, cols;
  int32_t pitch;               /* bytes of a row of depth: a multiple of 4, at least 4 * cols */
  int32_t pose_stride;         /* poses per sequence */
  int32_t nx, ny, nz;          /* voxels of a sequence's volume */
  int32_t reserved0;
  const float* origin;         /* in [batch][4] the world position of the corner of voxel (0, 0, 0); the fourth float is unread */
  const float* volume;         /* in [batch][nz][ny][nx][2] (tsdf, weight), 16-byte aligned */
  const float* pose;           /* in [batch][pose_stride][16] */
  const int32_t* view_index;   /* in [batch][views] the pose of view r (NULL allowed: r) */
  const int32_t* n_views;      /* in [batch] (NULL allowed: views) */
  float* depth;                /* out [batch][views][rows][pitch] metres of z depth, 0 = no surface */
  float* normal;               /* out [batch][views][rows][cols][4], 16-byte aligned (NULL allowed) */
  int32_t* n_hit;              /* out [batch][views] pixels with depth > 0 (NULL allowed) */
  int32_t* n_skipped;          /* out [batch] */
  int32_t* status;             /* out [batch] */
  void* workspace;             /* prs_tsdf_raycast_workspace_bytes(batch, views), 16-byte aligned */
  void* reserved[2];
} prs_tsdf_raycast_batch;

/* device pointers, asynchronous on the context's stream */
PRS_API int prs_tsdf_raycast_batch_run(prs_context* ctx, const prs_tsdf_raycast_params* params, const prs_tsdf_raycast_batch* batch);
/* bytes of the workspace, 0 for sizes the call refuses */
PRS_API uint64_t prs_tsdf_raycast_workspace_bytes(int32_t batch, int32_t views);
/* sizeof prs_tsdf_raycast_params, prs_tsdf_raycast_batch as the library was compiled (bindings check) */
PRS_API void prs_tsdf_raycast_struct_sizes(uint64_t* sizes2);

#ifdef __cplusplus
}
#endif

#endif /* PROSLAM_HIP_TSDF_RAYCAST_H */
