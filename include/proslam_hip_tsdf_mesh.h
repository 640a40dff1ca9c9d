/* proslam_hip_tsdf_mesh.h -- a TSDF volume as an indexed quad mesh on the device (gfx950): the sixth public header of
 * libproslam_hip.so.
 *
 * include/proslam_hip.h is pinned to the layout of PRS_ABI_VERSION 104; what this header declares joins it, as it stands here, at
 * the next layout bump, and this file then only includes the main header.  Until then: the entry points below are exported from
 * the same library, use PRS_API, the status codes and prs_context of the main header and prs_tsdf_params of the third header, and
 * have their own size query (prs_tsdf_mesh_struct_sizes) in the place of prs_abi_check.  Every struct ends in reserved words:
 * memset it to 0 before filling it in.
 */
#ifndef PROSLAM_HIP_TSDF_MESH_H
#define PROSLAM_HIP_TSDF_MESH_H

#include "proslam_hip_tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ================================================================================================
 * TSDF mesh: the volume prs_tsdf_integrate_batch_run fuses (include/proslam_hip_tsdf.h: (tsdf, weight) a voxel), turned into one
 * indexed mesh of quads per sequence by SURFACE NETS (Gibson 1998), the dual of marching cubes: one vertex in every cube of eight
 * voxels that the surface passes through, one quad around every grid edge that crosses it.  The crossings are exactly the rows of
 * prs_tsdf_surface_batch_run, in its order and with its `cell` ids, so a face can be joined to a surface row.
 *
 * BUILD-DEFINED, like the other dense stages: the reference has no dense stage.  tests/tsdf_mesh_ref.py restates the rule in numpy
 * and the kernels equal that byte for byte.  All arithmetic is explicit two-operand float32 in the order written,
 * -ffp-contract=off, division and sqrtf correctly rounded, denormals kept.  Of params only voxel_size and min_weight are read.
 *
 * ---- prs_tsdf_mesh_batch_run: vertex, normal, quad, cube, edge (out) <- volume (in) ----
 * With (n0, n1, n2) = (nx, ny, nz), u_e the unit step along axis e and lin(i, j, k) = (k * ny + j) * nx + i:
 *   crossing   a TAKEN CROSSING (a, e) is the surface call's: voxel a, axis e, n = a + u_e in the grid, a and n both in band
 *              (w >= min_weight && fabsf(tsdf) < 1.0f) and (t_a < 0.0f) != (t_n < 0.0f).  Its id is the surface call's cell,
 *              3 * lin(a) + e; its point P the first three floats of the surface call's xyz row; its normal N the four floats of
 *              the surface call's normal row (csrc/prs_tsdf_cross.h holds the one expression both calls run).
 *   cube       q = (i, j, k) exists for 0 <= i < nx - 1, 0 <= j < ny - 1, 0 <= k < nz - 1: a grid with an axis of one voxel has
 *              none.  Its twelve edges are the (a, e) with a_e = q_e and a_d in {q_d, q_d + 1} on the two other axes.  It is ACTIVE
 *              iff at least one of them is a taken crossing; m = how many are (1 .. 12).
 *   vertex     of an active cube: its taken crossings in ascending id; per coordinate s_d = +0.0f, then s_d = s_d + P_d for each;
 *              the row is (s0 / (float) m, s1 / (float) m, s2 / (float) m, (float) m).
 *   normal     the same crossings, skipping those whose N has fourth float 0: g_d = +0.0f, then g_d = g_d + N_d for each;
 *              len2 = (g0 * g0 + g1 * g1) + g2 * g2.  With len2 > 0 && len2 <= FLT_MAX the row is
 *              (g0 / sqrtf(len2), g1 / sqrtf(len2), g2 / sqrtf(len2), 1.0f), otherwise (0, 0, 0, 0).
 *   order      the vertices are numbered in raster order of their cubes (k outer, then j, then i): r(q) is the rank of q among
 *              ALL active cubes of the sequence, whether or not its row fits.  cube row = lin(q).
 *              n_vertices_total[b] = the active cubes, n_vertices[b] = min(n_vertices_total[b], vertex_stride); the rows from
 *              n_vertices[b] on are left untouched.
 *   quad       the taken crossings in ascending id, with b = (e + 1) mod 3 and c = (e + 2) mod 3.  The crossing is INTERIOR iff
 *              1 <= a_b <= n_b - 2 and 1 <= a_c <= n_c - 2: the four cubes around the edge then exist and each is active.  Other
 *              crossings emit nothing.  With q00 = a - u_b - u_c, q10 = a - u_c, q11 = a, q01 = a - u_b the row is
 *              (r(q00), r(q10), r(q11), r(q01)) when t_a < 0.0f and (r(q00), r(q01), r(q11), r(q10)) otherwise: counter-clockwise
 *              seen from the observed free side, so the face normal agrees with the surface call's normal.  The triangles of a
 *              quad are always (v0, v1, v2) and (v0, v2, v3).  edge row = the crossing's id.
 *              n_quads_total[b] = the interior crossings, n_quads[b] = min(n_quads_total[b], quad_stride); the rows beyond are
 *              left untouched.
 *   status     status[b] is PRS_ERR_CAPACITY when n_vertices_total[b] > vertex_stride or n_quads_total[b] > quad_stride, else
 *              PRS_OK.  Only then may a quad name a vertex row that was not written.
 *   count only vertex and quad both NULL: the two totals as above, n_vertices[b] = n_quads[b] = 0, status[b] = PRS_OK, nothing
 *              else written (normal, cube and edge must then be NULL too).
 * The totals fit an int32 by construction: vertices <= voxels, quads <= 3 * voxels.
 * Call-level (return value, nothing launched, outputs untouched): PRS_ERR_NULL (a struct, origin, volume, one of the five
 * per-sequence outputs or workspace unset; only one of vertex and quad set; normal, cube or edge set without them);
 * PRS_ERR_RANGE (batch, nx, ny or nz < 1; vertex_stride or quad_stride < 1 with outputs set; voxel_size not finite or <= 0;
 * min_weight not finite); PRS_ERR_UNSUPPORTED (volume, vertex, normal, quad or workspace not 16-byte aligned, another array not
 * 4-byte aligned; nx * ny * nz beyond (2^31 - 1) / 3; a launch beyond 2^32 - 1 work-items, which is 2^24 - 1 workgroups of 256
 * threads: prs_launch_fits).
 * Deterministic, without a float atomic: FOUR plain launches on the context's stream, TWO for the count-only call.  count (a
 * workgroup per chunk of 1024 voxels that follow one another in raster order, the surface call's chunks: a lane reads the eight
 * corners of its cube in place, reduces them to a band bit and a sign bit each, and from those takes the cube's twelve edges and
 * its own three; wave ballots, two counts a chunk into the workspace), scan (a workgroup a sequence: both rows of chunk bases by
 * csrc/prs_compact.h, the four counts and the status), vertices (the same ballots give every active cube its rank, which goes
 * into an int32 per voxel of the workspace; the lanes of active cubes alone walk their crossings) and quads (the same ballots give
 * every interior crossing its row; four ranks are gathered from that map, which is read only where this call wrote it, and the
 * row is one 16-byte store).  Byte indexing into volume, the outputs and the workspace is 64-bit.  No allocation, no
 * synchronisation, no host read: graph-capturable.
 *
 * Left out: marching cubes' one-vertex-per-edge mesh; resolving non-manifold edges (where a cube face has four crossing edges a
 * mesh edge is shared by four quads: the rule is still well defined); vertex placement by QEF / dual contouring; colour; mesh
 * simplification; welding across sequences; a host-pointer variant and a C++ adapter in plugin/.
 * ============================================================================================== */

/* device pointers */
typedef struct {
  int32_t batch;
  int32_t nx, ny, nz;          /* voxels of a sequence's volume */
  int32_t vertex_stride;       /* rows per sequence of vertex, normal and cube */
  int32_t quad_stride;         /* rows per sequence of quad and edge */
  const float* origin;         /* in [batch][4] the world position of the corner of voxel (0, 0, 0); the fourth float is unread */
  const float* volume;         /* in [batch][nz][ny][nx][2] (tsdf, weight), 16-byte aligned */
  float* vertex;               /* out [batch][vertex_stride][4], 16-byte aligned (NULL with quad NULL: count only) */
  float* normal;               /* out [batch][vertex_stride][4], 16-byte aligned (NULL allowed) */
  int32_t* quad;               /* out [batch][quad_stride][4] vertex rows of the sequence, 16-byte aligned */
  int32_t* cube;               /* out [batch][vertex_stride] (NULL allowed) */
  int32_t* edge;               /* out [batch][quad_stride] (NULL allowed) */
  int32_t* n_vertices;         /* out [batch] */
  int32_t* n_vertices_total;   /* out [batch] */
  int32_t* n_quads;            /* out [batch] */
  int32_t* n_quads_total;      /* out [batch] */
  int32_t* status;             /* out [batch] */
  void* workspace;             /* prs_tsdf_mesh_workspace_bytes(batch, nx, ny, nz), 16-byte aligned */
  void* reserved[3];
} prs_tsdf_mesh_batch;

/* device pointers, asynchronous on the context's stream */
PRS_API int prs_tsdf_mesh_batch_run(prs_context* ctx, const prs_tsdf_params* params, const prs_tsdf_mesh_batch* batch);
/* bytes of the workspace, 0 for sizes the call refuses */
PRS_API uint64_t prs_tsdf_mesh_workspace_bytes(int32_t batch, int32_t nx, int32_t ny, int32_t nz);
/* sizeof prs_tsdf_mesh_batch as the library was compiled (bindings check) */
PRS_API void prs_tsdf_mesh_struct_sizes(uint64_t* sizes1);

#ifdef __cplusplus
}
#endif

#endif /* PROSLAM_HIP_TSDF_MESH_H */
