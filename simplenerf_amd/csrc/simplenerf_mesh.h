/*
 * simplenerf_mesh.h -- the surface export of the simplenerf_hip library: depth maps that are already on the device are fused into a
 * truncated signed distance volume (snerf_tsdf_integrate), a triangle mesh is extracted from the volume by marching tetrahedra
 * (snerf_mesh_count, snerf_mesh_emit), and any point set -- the mesh's vertices -- is coloured from the frames (snerf_colour_points).
 * Declared beside include/simplenerf_hip.h like simplenerf_fuse.h (the prototypes of the pinned header groups do not change).  Same
 * conventions: status codes, snerf_last_error, device pointers, enqueue-only on `stream`, no allocation, no synchronisation, every
 * check before the first launch.  ABI version 10 is unchanged -- a caller checks that the symbol exists.
 *
 * Cameras, pixels and depths are those of simplenerf_fuse.h: integer pixel coordinates, x = column, y = row; z-depths in the
 * extrinsics' units; the camera table of SNERF_FUSE_CAMERA_DOUBLES doubles per view, unchanged.  All device arithmetic is fp64 (fp32
 * inputs are widened on load), no fused multiply-add, no atomics: every output element has one owning thread, and the same input
 * gives the same bits on every call.
 *
 * THE GRID.  nx, ny, nz >= 1 nodes; node (i, j, k) sits at p_a = lo_a + voxel_size . i_a (one fp64 product, one sum).  Arrays are
 * shaped (nz, ny, nx); the node index is n = (k . ny + j) . nx + i.  7 . nx . ny . nz <= 2^31 - 1 (SNERF_MESH_KEYS_PER_NODE keys a
 * node, numbered by an int); above that every call returns SNERF_E_UNSUPPORTED.
 *
 * THE LOOKUP of a point P in view u (the fuse's, in its order of operations):
 *   c_a = ((E[a][0] P_0 + E[a][1] P_1) + E[a][2] P_2) + E[a][3].  If not c_z > 0 the view does not see P.
 *   q_a = (K[a][0] c_0 + K[a][1] c_1) + K[a][2] c_2;  px = q_0 / q_2, py = q_1 / q_2;  ix = rint(px), iy = rint(py), ties to even.
 *   The pixel must satisfy 0 <= ix < width and 0 <= iy < height, tested on the floating-point values before any conversion to an
 *   integer, so a non-finite or enormous projection can never index memory.
 *   d = depth[u, iy, ix] must be VALID: finite, d > 0, and the mask byte (if a mask is given) non-zero.
 */
#ifndef SIMPLENERF_MESH_H
#define SIMPLENERF_MESH_H

#include <stddef.h>

#include "simplenerf_hip.h"
#include "simplenerf_fuse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_MESH_KEYS_PER_NODE 7     /* the edge types that start at a node */

/* snerf_tsdf_integrate: `views` depth maps -> a truncated signed distance per node and the number of views that gave one.
 *   depth     device (views, height, width) float
 *   mask      device (views, height, width) bytes, or NULL
 *   cameras   device (views, SNERF_FUSE_CAMERA_DOUBLES) double
 *   voxel_size > 0, lo_x, lo_y, lo_z, nx, ny, nz: the grid;  truncation mu > 0
 *   tsdf      device (nz, ny, nx) float;  weight  device (nz, ny, nx) bytes
 *
 * THE RULE per node P, views u in ascending order: look P up in view u; s = d - c_z; skip the view unless s >= -mu (the node lies
 * behind the surface this view sees; a NaN is skipped too); t = min(1, s / mu); sum += t (fp64, sequentially), count += 1.
 * tsdf = (float)(sum / count) when count > 0, else 1.0f;  weight = count (views <= SNERF_FUSE_MAX_VIEWS keeps it a byte).
 * One thread owns one node, x fastest (one launch).
 *
 * Errors.  views, height or width negative, views > SNERF_FUSE_MAX_VIEWS, voxel_size or truncation not a finite number > 0, a bound
 * that is not finite, an extent < 1, tsdf or weight NULL, or with views . height . width > 0 depth or cameras NULL: SNERF_E_INVALID.
 * views . height . width > 2^31 - 1 or a grid above the limit: SNERF_E_UNSUPPORTED.  views . height . width == 0 gives every weight
 * 0 and every tsdf 1. */
int snerf_tsdf_integrate(const float* depth, const unsigned char* mask, const double* cameras, int views, int height, int width,
                         double voxel_size, double lo_x, double lo_y, double lo_z, int nx, int ny, int nz, double truncation, float* tsdf,
                         unsigned char* weight, snerf_stream_t stream);

/* snerf_mesh_count, snerf_mesh_emit: marching tetrahedra over the volume.
 *   tsdf, weight, voxel_size, lo, nx, ny, nz: a volume as snerf_tsdf_integrate writes it;  min_weight 1 .. 255
 *   counts    device long long[2]: [0] the number of vertices Nv, [1] the number of triangles Nt.  snerf_mesh_count writes them;
 *             snerf_mesh_emit reads them as the sizes of its outputs and never writes a row at or past them
 *   vertices  device (Nv, 3) float;  triangles  device (Nt, 3) int: vertex numbers
 *   workspace device scratch of at least snerf_mesh_workspace_bytes(nx, ny, nz), 256-byte aligned; no initial state for
 *             snerf_mesh_count, which leaves its scans there; snerf_mesh_emit takes the same arguments and that workspace
 *
 * THE RULE
 * A node is NEGATIVE iff tsdf < 0.  A cell, with origin node (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, is COMPLETE iff all eight
 * of its nodes have weight >= min_weight.  Only complete cells produce triangles.
 * A cell splits into the six Kuhn tetrahedra: tetrahedron T (0..5) belongs to the T-th permutation (a, b, c) of the axes in
 * lexicographic order (xyz, xzy, yxz, yzx, zxy, zyx); its vertices are m0 = the cell origin, m1 = m0 + e_a, m2 = m1 + e_b,
 * m3 = m2 + e_c.  Its case is the 4-bit number whose bit m is set when vertex m is negative.
 * Triangles are named by tetrahedron edges (m, m'), m < m'.  One vertex m alone of its sign: one triangle on the edges (m, o) for
 * the other three o ascending.  Two negative n0 < n1 and two positive p0 < p1: the quad q = n0p0, n0p1, n1p1, n1p0, as the
 * triangles (q0, q1, q2) and (q0, q2, q3).  The winding is fixed per (tetrahedron, case), never decided from the data: with node
 * values of +-1 (vertices at edge midpoints), (v1 - v0) x (v2 - v0) has a positive dot product with (mean of the positive nodes -
 * mean of the negative nodes), else the triangle's last two vertices are swapped.  csrc/mesh_tables.h holds the 6 x 16 table.
 * A VERTEX is an edge of the grid.  Of its two nodes A is the one earlier on the path (componentwise <=); its key is
 * 7 . n(A) + type, the type from B - A: (1,0,0) 0, (0,1,0) 1, (0,0,1) 2, (1,1,0) 3, (1,0,1) 4, (0,1,1) 5, (1,1,1) 6.  An edge is a
 * mesh vertex iff its nodes differ in sign and at least one complete cell contains it (of the four cells round an axis edge, the
 * two of a face diagonal, the one of a body diagonal).  Vertices are numbered in ascending key order.  Position:
 *   s = (double)t_A / ((double)t_A - (double)t_B);  P_a = p_A,a + s . (p_B,a - p_A,a), rounded to float.
 * Triangles come in ascending (cell origin node index, tetrahedron, the case's own order).
 * Both compactions are count per tile of 2048 nodes, scan, scatter: snerf_mesh_count is five launches, snerf_mesh_emit one.
 * A grid with an extent of 1, or without a complete cell, gives 0 and 0.
 *
 * Errors.  voxel_size not a finite number > 0, a bound that is not finite, an extent < 1, min_weight outside 1 .. 255, a NULL
 * pointer, a workspace that is not 256-byte aligned or counts that is not 8-byte aligned: SNERF_E_INVALID.  A grid above the limit:
 * SNERF_E_UNSUPPORTED.  The query returns 0 for a grid the calls reject. */
long long snerf_mesh_workspace_bytes(int nx, int ny, int nz);
int snerf_mesh_count(const float* tsdf, const unsigned char* weight, double voxel_size, double lo_x, double lo_y, double lo_z, int nx,
                     int ny, int nz, int min_weight, long long* counts, void* workspace, snerf_stream_t stream);
int snerf_mesh_emit(const float* tsdf, const unsigned char* weight, double voxel_size, double lo_x, double lo_y, double lo_z, int nx,
                    int ny, int nz, int min_weight, const long long* counts, float* vertices, int* triangles, void* workspace,
                    snerf_stream_t stream);

/* snerf_colour_points: a colour per point from the views that see it.
 *   points    device (count, 3) float, widened to fp64
 *   depth, image (views, height, width, 3) bytes, mask (or NULL), cameras: as snerf_fuse_depth_maps takes them
 *   colour_tolerance >= 0, in scene units
 *   colours   device (count, 3) bytes;  agreeing  device (count) bytes
 *
 * THE RULE per point, views u in ascending order: look the point up in view u; the view AGREES iff |c_z - d| <= colour_tolerance.
 * Each colour channel is (2 . sum + n) div (2 . n) over the n agreeing views' pixels image[u, iy, ix], integers only; (0, 0, 0) with
 * n = 0.  agreeing = n.  One thread owns one point (one launch).
 *
 * Errors.  count, views, height or width negative, views > SNERF_FUSE_MAX_VIEWS, colour_tolerance not >= 0, or with count > 0 points,
 * colours or agreeing NULL, or with count > 0 and views . height . width > 0 depth, image or cameras NULL: SNERF_E_INVALID.  count or
 * views . height . width > 2^31 - 1: SNERF_E_UNSUPPORTED.  count == 0 enqueues nothing. */
int snerf_colour_points(const float* points, long long count, const float* depth, const unsigned char* image, const unsigned char* mask,
                        const double* cameras, int views, int height, int width, double colour_tolerance, unsigned char* colours,
                        unsigned char* agreeing, snerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLENERF_MESH_H */
