/*
 * simplenerf_fuse.h -- the geometry export of the simplenerf_hip library: depth maps that are already on the device leave it as one
 * consistency-filtered, coloured point cloud (snerf_fuse_depth_maps), optionally thinned to one point per occupied voxel
 * (snerf_voxel_thin).  Declared beside include/simplenerf_hip.h like simplenerf_png.h and simplenerf_jpeg.h (the prototypes of the
 * pinned header groups do not change).  Same conventions: status codes, snerf_last_error, device pointers, enqueue-only on `stream`,
 * no allocation, no synchronisation, every check before the first launch.  ABI version 10 is unchanged -- a caller checks that the
 * symbol exists.
 *
 * Conventions of both calls (those of snerf_visibility_mask_* and snerf_warp_*): integer pixel coordinates, x = column, y = row;
 * z-depths in the extrinsics' units; extrinsics E 4x4 world-to-camera, intrinsics K 3x3, inverted and composed by the caller on the
 * host in float64.  All device arithmetic is fp64 (fp32 inputs are widened on load), no fused multiply-add, no atomic on a float:
 * the same input gives the same bits on every call.
 */
#ifndef SIMPLENERF_FUSE_H
#define SIMPLENERF_FUSE_H

#include <stddef.h>

#include "simplenerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_FUSE_CAMERA_DOUBLES 42   /* per view, row-major: inv(K) 3x3 | rows 0..2 of inv(E) 3x4 | rows 0..2 of E 3x4 | K 3x3 */
#define SNERF_FUSE_MAX_VIEWS 255       /* the number of agreeing views of a point is a byte */

/* snerf_fuse_depth_maps: `views` depth maps with their colour frames -> the points that at least `min_views` OTHER views confirm.
 *   depth     device (views, height, width) float
 *   image     device (views, height, width, 3) bytes
 *   mask      device (views, height, width) bytes, or NULL
 *   cameras   device (views, SNERF_FUSE_CAMERA_DOUBLES) double
 *   depth_error_threshold  tau >= 0
 *   min_views 0 .. views - 1
 *   points    device (views * height * width, 3) float: the first N rows are written
 *   colours   device (views * height * width, 3) bytes: the first N rows are written
 *   agreeing  device (views * height * width) bytes: the first N are written, the number of agreeing views of each kept point
 *   kept      device long long: N
 *   workspace device scratch of at least snerf_fuse_depth_maps_workspace_bytes(...), 256-byte aligned; no initial state
 *
 * THE RULE
 * Source pixel (v, y, x) is VALID iff d = depth[v, y, x] is finite, d > 0, and the mask (if given) is non-zero.
 * Its point is P = inv(E_v)[:3] . [d . inv(K_v) . (x, y, 1); 1], in this order of operations:
 *   r_a = (Ki[a][0] x + Ki[a][1] y) + Ki[a][2];  c_a = d r_a;  P_a = ((Ei[a][0] c_0 + Ei[a][1] c_1) + Ei[a][2] c_2) + Ei[a][3]
 * For every other view u (ascending, u != v):
 *   c = E_u[:3] . [P; 1] (the same order as P_a).  If not c_z > 0, the view does not see it.
 *   q = K_u . c, q_a = (K[a][0] c_0 + K[a][1] c_1) + K[a][2] c_2;  px = q_0 / q_2, py = q_1 / q_2.
 *   ix = rint(px), iy = rint(py), fp64, ties to even.
 *   The pixel must satisfy 0 <= ix < width and 0 <= iy < height.  This is tested on the floating-point values before any conversion to
 *   an integer, so a non-finite or enormous projection can never index memory.
 *   d_u = depth[u, iy, ix] must itself be valid (its mask byte included).
 *   View u AGREES iff |c_z - d_u| <= tau . d_u.
 * The pixel is KEPT iff it is valid and at least min_views other views agree.
 * Outputs: the kept points as float (P rounded to nearest), their colours image[v, y, x], their numbers of agreeing views, and N, in
 * ascending (v, y, x) order (an order-preserving compaction: count per tile of 2048 pixels, scan, scatter -- four launches).
 *
 * Errors.  views, height or width negative, views > SNERF_FUSE_MAX_VIEWS, tau not >= 0, min_views outside 0 .. max(views - 1, 0), or
 * with views * height * width > 0 a NULL pointer (mask may be NULL) or a workspace that is not 256-byte aligned: SNERF_E_INVALID.
 * views * height * width > 2^31 - 1: SNERF_E_UNSUPPORTED.  views * height * width == 0 enqueues NOTHING (`kept` is not written) and
 * returns SNERF_OK.  The query returns 0 for arguments the call rejects or enqueues nothing for. */
long long snerf_fuse_depth_maps_workspace_bytes(int views, int height, int width);
int snerf_fuse_depth_maps(const float* depth, const unsigned char* image, const unsigned char* mask, const double* cameras, int views,
                          int height, int width, double depth_error_threshold, int min_views, float* points, unsigned char* colours,
                          unsigned char* agreeing, long long* kept, void* workspace, snerf_stream_t stream);

/* snerf_voxel_thin: one point per occupied voxel of a regular grid.
 *   points    device (count, 3) float;  colours  device (count, 3) bytes
 *   voxel_size > 0;  lo_x, lo_y, lo_z: the grid's corner (the per-axis minimum of the points);  nx, ny, nz >= 1: its extents in
 *   voxels, nx * ny * nz <= 2^31 - 1.  The caller computes these.
 *   thinned_points (count, 3) float, thinned_colours (count, 3) bytes, counts (count) int: the first M rows are written
 *   runs      device long long: M, the number of occupied voxels
 *   workspace device scratch of at least snerf_voxel_thin_workspace_bytes(...), 256-byte aligned; no initial state
 *
 * THE RULE
 * Per point, i_a = floor(((double)p_a - lo_a) / voxel_size); int key (i_z . ny + i_y) . nx + i_x.  (An index outside 0 .. n_a - 1 --
 * bounds that are not those of the points -- is moved to the nearer end, a NaN to 0: a key only orders, it never indexes.)
 * Stable sort through snerf_sort_keys_with_order over just the bits in use.  Per run of equal keys:
 *   the position is (float)(sum (double)p / count), the sum taken sequentially in ascending source order;
 *   each colour channel is (2 . sum c + count) div (2 . count), integers only;
 *   the count is an int.
 * Runs are written in ascending key order.  One thread walks one run: a run of r points is r dependent additions (the rule's
 * sequential sum), which bounds the call when nearly all points share a voxel.
 *
 * Errors.  count < 0, voxel_size not a finite number > 0, a bound that is not finite, an extent < 1, or with count > 0 a NULL pointer
 * or a workspace that is not 256-byte aligned: SNERF_E_INVALID.  count or nx * ny * nz > 2^31 - 1: SNERF_E_UNSUPPORTED.  count == 0
 * writes runs = 0 (one launch).  The query returns 0 for arguments the call rejects and for count == 0. */
long long snerf_voxel_thin_workspace_bytes(long long count, int nx, int ny, int nz);
int snerf_voxel_thin(const float* points, const unsigned char* colours, long long count, double voxel_size, double lo_x, double lo_y,
                     double lo_z, int nx, int ny, int nz, float* thinned_points, unsigned char* thinned_colours, int* counts,
                     long long* runs, void* workspace, snerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLENERF_FUSE_H */
