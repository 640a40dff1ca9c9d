/* proslam_hip_tsdf.h -- TSDF fusion of depth images on the device (gfx950): the third public header of libproslam_hip.so.
 *
 * include/proslam_hip.h is pinned to the layout of PRS_ABI_VERSION 104; what this header declares joins it, as it stands here, at
 * the next layout bump, and this file then only includes the main header.  Until then: the entry points below are exported from
 * the same library, use PRS_API, the status codes, prs_context and PRS_DEPTH_U16 / PRS_DEPTH_F32 of the main header, and have
 * their own size query (prs_tsdf_struct_sizes) in the place of prs_abi_check.  Every struct ends in reserved words: memset it to 0
 * before filling it in.
 */
#ifndef PROSLAM_HIP_TSDF_H
#define PROSLAM_HIP_TSDF_H

#include "proslam_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ================================================================================================
 * TSDF fusion: the depth images prs_depth_cloud_batch_run reads (the sensor's, a matcher's, or the consistency filter's out),
 * averaged along the viewing ray into a truncated signed distance volume per sequence (Curless and Levoy 1996; KinectFusion), and
 * the zero crossings of that volume as points with normals.  Each voxel holds (tsdf, weight): the running weighted mean of the
 * signed distance to the observed surface in units of `truncation`, positive in front of it, and the number of observations,
 * saturating at max_weight.  A volume of all-zero bytes is an empty volume: weight 0 means never observed.
 *
 * BUILD-DEFINED, like the other dense stages: the reference has no dense stage.  tests/tsdf_ref.py restates the rule in numpy and
 * the kernels equal that byte for byte.  All arithmetic is explicit two-operand float32 in the order written, -ffp-contract=off,
 * division and sqrtf correctly rounded, denormals kept; se3_mul, se3_inverse and se3_apply are those of csrc/prs_se3.h, whose
 * expression order is the specification.
 *
 * ---- prs_tsdf_integrate_batch_run: volume (in/out) <- depth images ----
 * Per sequence b and voxel (i, j, k), i < nx fastest, with (o0, o1, o2) = origin[b] the world position of the corner of voxel
 * (0, 0, 0), the centre is
 *   c = (o0 + ((float) i + 0.5f) * voxel_size, o1 + ((float) j + 0.5f) * voxel_size, o2 + ((float) k + 0.5f) * voxel_size)
 * and, with (tsdf, w) = volume[b][k][j][i], for the images f = 0 .. n_images[b] - 1 (frames when n_images is NULL) IN THAT ORDER:
 *   frame        kf = frame_index[b][f], or f when frame_index is NULL.  The frame is skipped, exactly as the dense cloud skips it,
 *                and counted in n_skipped[b], when kf lies outside [0, pose_stride) or one of the twelve top-row entries of
 *                pose[b][kf] is not finite.  Otherwise T = se3_mul(pose[b][kf], sensor_in_robot) and Ti = se3_inverse(T).
 *   camera point q = se3_apply(Ti, c), z = q2.  Go on iff z > 0 && z >= range_min && z <= range_max (which drops NaN).
 *   pixel        uf = floorf((q0 / z * fx + cx) + 0.5f), vf = floorf((q1 / z * fy + cy) + 0.5f).  Go on iff
 *                uf >= 0 && uf < (float) cols && vf >= 0 && vf < (float) rows; u = (int) uf, v = (int) vf.
 *   depth        raw = the element (v, u) of image (b, f) as a float.  Go on iff raw > 0 and, with
 *                d = depth_scaling_factor_to_meters * raw, d >= range_min && d <= range_max: the cloud's test.
 *   distance     sdf = d - z.  Go on iff sdf >= -truncation.  t = sdf / truncation, replaced by 1.0f when t > 1.0f.
 *   update       w1 = w + 1.0f; tsdf = (tsdf * w + t) / w1; w = w1, replaced by max_weight when w1 > max_weight.
 * volume[b][k][j][i] = (tsdf, w) afterwards.  A voxel that no image reaches keeps its bytes, and fusing images 0 .. 3 in one call
 * equals fusing 0 .. 1 and then 2 .. 3 in two calls, byte for byte.
 *   counts       n_updates[b][f] (optional) = the voxels image f updated (integer adds: the same whatever their order), written
 *                for every f < frames: 0 for a skipped frame and for the frames from n_images[b] on.  n_skipped[b] as above.
 * status[b]: PRS_ERR_RANGE when n_images[b] lies outside [0, frames]; nothing of that sequence is then written but
 * n_skipped[b] = 0.  Otherwise PRS_OK.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, depth, pose, origin, volume, n_skipped,
 * status or workspace unset); PRS_ERR_RANGE (batch, frames, rows, cols, pose_stride, nx, ny or nz < 1; pitch below cols elements
 * or not a multiple of the element size; a parameter that is not finite -- sensor_in_robot included, min_weight excluded: this
 * call does not read it --, a scale <= 0, range_min < 0 or range_min > range_max, voxel_size <= 0, truncation <= 0,
 * max_weight < 1); PRS_ERR_UNSUPPORTED (an unknown depth_type; volume or workspace not 16-byte aligned, depth not aligned to its
 * element, another array not 4-byte aligned; nx * ny * nz beyond (2^31 - 1) / 3, rows * cols or batch * frames beyond 2^31 - 1; a
 * launch beyond 2^32 - 1 work-items, which is 2^24 - 1 workgroups of 256 threads: prs_launch_fits).
 * Two plain launches on the context's stream.  head (a workgroup a sequence, a thread an image): status, n_skipped, 0 into
 * n_updates, and Ti with a served flag for every image into the workspace.  bricks (a workgroup of 256 threads per brick of
 * 32 x 4 x 4 voxels of one sequence, two voxels a lane, consecutive lanes on consecutive i): a lane keeps its voxels' (tsdf, w) in
 * registers across the whole frame loop, so the volume's traffic is one 8-byte load and at most one 8-byte store a voxel and call,
 * whatever `frames` is; Ti comes through LDS, 32 images at a time, as a wave-uniform read; the depth reads are gathers; n_updates
 * costs a ballot count a wave and one integer atomic add a workgroup and image.  No brick is rejected against a frustum: every
 * voxel runs the rule itself.  Byte indexing into volume is 64-bit.  No allocation, no synchronisation, no host read:
 * graph-capturable.
 *
 * ---- prs_tsdf_surface_batch_run: points with normals <- volume (in) ----
 * A voxel is OBSERVED iff w >= min_weight, and IN BAND iff it is observed and fabsf(tsdf) < 1.0f.  The voxels are walked in raster
 * order (k outer, then j, then i); per voxel a the axes in the order e = 0 (x), 1 (y), 2 (z), with n the next voxel along e:
 *   crossing     taken iff n lies in the grid, a and n are both in band and (t_a < 0.0f) != (t_n < 0.0f).  The band test keeps the
 *                jump from truncated free space (tsdf 1) to a surface seen edge-on from becoming a phantom sheet.
 *   point        s = t_a / (t_a - t_n); the row is a's centre c (above) with p_e = c_e + s * voxel_size; its fourth float is the
 *                smaller of w_a and w_n (w_n < w_a ? w_n : w_a).
 *   normal       taken at g = n when fabsf(t_n) < fabsf(t_a), else a (a tie goes to a).  For each axis, hi = the tsdf of g's next
 *                voxel along it when that voxel lies in the grid and is observed, else g's own tsdf; lo the same on the other
 *                side; m = hi - lo.  len2 = (m0 * m0 + m1 * m1) + m2 * m2.  With len2 > 0 && len2 <= FLT_MAX the row is
 *                (m0 / sqrtf(len2), m1 / sqrtf(len2), m2 / sqrtf(len2), 1.0f), otherwise (0, 0, 0, 0).  The normal points to the
 *                observed free side, as the depth normals face the camera.
 *   cell         3 * (the linear index (k * ny + j) * nx + i of a) + e.
 *   counts       n_total[b] = the crossings of the sequence, n_out[b] = min(n_total[b], out_stride); the first n_out[b] crossings
 *                are rows 0 .. n_out[b] - 1 of xyz, normal and cell, the rows from n_out[b] on are left untouched, and status[b]
 *                is PRS_ERR_CAPACITY when n_total[b] > out_stride, else PRS_OK.  xyz NULL is the count-only call: n_total as
 *                above, n_out[b] = 0, status[b] = PRS_OK, nothing else written (normal and cell must then be NULL too).  There is
 *                no n_base.
 * Call-level: PRS_ERR_NULL (a struct, origin, volume, n_out, n_total, status or workspace unset, or normal or cell set without
 * xyz); PRS_ERR_RANGE (batch, nx, ny or nz < 1, out_stride < 1 with xyz set, voxel_size not finite or <= 0, min_weight not
 * finite); PRS_ERR_UNSUPPORTED (volume, xyz, normal or workspace not 16-byte aligned, another array not 4-byte aligned;
 * nx * ny * nz beyond (2^31 - 1) / 3; a launch beyond the limit above).  Of params only voxel_size and min_weight are read.
 * Deterministic, without a float atomic: count (a workgroup per chunk of 1024 voxels that follow one another in raster order,
 * which is the order of the rows: wave ballots, one count a chunk into the workspace), scan (a workgroup a sequence: the chunk
 * bases, csrc/prs_compact.h) and scatter (the same ballots give every crossing its row); the neighbours are read in place, a
 * one-voxel halo around the chunk.  Three plain launches, two for the count-only call; graph-capturable.
 *
 * Left out: ray-length rather than z distance; observation weights other than 1; trilinear depth sampling; colour; a hashed or
 * sparse volume; a triangle mesh (marching cubes); a volume that moves with the camera; a host-pointer variant and a C++ adapter in
 * plugin/.
 * ============================================================================================== */
typedef struct {
  int32_t depth_type;                    /* PRS_DEPTH_U16 or PRS_DEPTH_F32 */
  float depth_scaling_factor_to_meters;  /* finite and > 0 */
  float fx, fy, cx, cy;                  /* the depth camera's matrix */
  float range_min, range_max;            /* metres, finite, 0 <= range_min <= range_max */
  float sensor_in_robot[16];             /* row-major; the identity when the poses are the camera's */
  float voxel_size;                      /* metres, finite, > 0 */
  float truncation;                      /* metres, finite, > 0 */
  float max_weight;                      /* finite, >= 1 */
  float min_weight;                      /* finite; read by the surface call alone */
  int32_t reserved[4];
} prs_tsdf_params;

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t frames;              /* images per sequence */
  int32_t rows, cols;
  int32_t pitch;               /* bytes, a multiple of the depth element's size */
  int32_t pose_stride;         /* poses per sequence */
  int32_t nx, ny, nz;          /* voxels of a sequence's volume */
  int32_t reserved0;
  const void* depth;           /* in [batch][frames][rows][pitch] */
  const int32_t* n_images;     /* in [batch] (NULL allowed: frames) */
  const float* pose;           /* in [batch][pose_stride][16], what prs_session_unroll_batch writes */
  const int32_t* frame_index;  /* in [batch][frames] the pose of image f (NULL allowed: f) */
  const float* origin;         /* in [batch][4] the world position of the corner of voxel (0, 0, 0); the fourth float is unread */
  float* volume;               /* in/out [batch][nz][ny][nx][2] (tsdf, weight), 16-byte aligned */
  int32_t* n_updates;          /* out [batch][frames] voxels the image updated (NULL allowed) */
  int32_t* n_skipped;          /* out [batch] */
  int32_t* status;             /* out [batch] */
  void* workspace;             /* prs_tsdf_workspace_bytes(batch, frames), 16-byte aligned */
  void* reserved[2];
} prs_tsdf_batch;

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t nx, ny, nz;
  int32_t out_stride;          /* rows per sequence of xyz, normal and cell */
  int32_t reserved0;
  const float* origin;         /* in [batch][4] */
  const float* volume;         /* in [batch][nz][ny][nx][2], 16-byte aligned */
  float* xyz;                  /* out [batch][out_stride][4], 16-byte aligned (NULL: count only) */
  float* normal;               /* out [batch][out_stride][4], 16-byte aligned (NULL allowed) */
  int32_t* cell;               /* out [batch][out_stride] (NULL allowed) */
  int32_t* n_out;              /* out [batch] */
  int32_t* n_total;            /* out [batch] */
  int32_t* status;             /* out [batch] */
  void* workspace;             /* prs_tsdf_surface_workspace_bytes(batch, nx, ny, nz), 16-byte aligned */
  void* reserved[3];
} prs_tsdf_surface_batch;

/* device pointers, asynchronous on the context's stream */
PRS_API int prs_tsdf_integrate_batch_run(prs_context* ctx, const prs_tsdf_params* params, const prs_tsdf_batch* batch);
PRS_API int prs_tsdf_surface_batch_run(prs_context* ctx, const prs_tsdf_params* params, const prs_tsdf_surface_batch* batch);
/* bytes of the workspaces, 0 for sizes the calls refuse */
PRS_API uint64_t prs_tsdf_workspace_bytes(int32_t batch, int32_t frames);
PRS_API uint64_t prs_tsdf_surface_workspace_bytes(int32_t batch, int32_t nx, int32_t ny, int32_t nz);
/* sizeof prs_tsdf_params, prs_tsdf_batch, prs_tsdf_surface_batch as the library was compiled (bindings check) */
PRS_API void prs_tsdf_struct_sizes(uint64_t* sizes3);

#ifdef __cplusplus
}
#endif

#endif /* PROSLAM_HIP_TSDF_H */
