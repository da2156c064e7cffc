/*
 * simplenerf_field.h -- the density field of a model as a level-set volume, in the simplenerf_hip library: the nodes of a grid, or
 * any point set, are mapped into the space the model's MLP reads and marked with the views that saw them
 * (snerf_field_grid_points, snerf_field_point_views); the densities snerf_mlp_forward returns at those points become the signed
 * volume that snerf_mesh_count / snerf_mesh_emit mesh (snerf_field_values).  No frame is rendered.  Declared beside
 * include/simplenerf_hip.h like simplenerf_mesh.h (the prototypes of the pinned header groups do not change).  Same conventions:
 * status codes, snerf_last_error, device pointers, enqueue-only on `stream`, no allocation, no synchronisation, every check before
 * the first launch.  ABI version 10 is unchanged -- a caller checks that the symbol exists.
 *
 * Cameras are those of simplenerf_fuse.h: the table of SNERF_FUSE_CAMERA_DOUBLES doubles per view, unchanged; integer pixel
 * coordinates, x = column, y = row.  The grid is that of simplenerf_mesh.h: node (i, j, k) at p_a = lo_a + voxel_size . i_a (one
 * fp64 product, one sum), node index n = (k . ny + j) . nx + i, 7 . nx . ny . nz <= 2^31 - 1.  All device arithmetic is fp64 (fp32
 * inputs are widened on load), no fused multiply-add, no atomics: every output element has one owning thread, and the same input
 * gives the same bits on every call.
 *
 * THE INPUT MAP of a point P of the scene frame (the frame of the extrinsics) to the point Q the MLP reads.
 *   ndc == 0:  Q = P.  cx, cy and near are not looked at.
 *   ndc != 0:  the model was trained on rays warped to normalised device coordinates (cameras look down -z).  The caller computes, in
 *   float64, cx = -1 / (W / (2 fx)), cy = -1 / (H / (2 fy)) from the frame size and the focal lengths the model was trained with,
 *   and passes the near plane's distance `near` > 0.
 *   P is IN FRONT iff P_z <= -near.  For a point in front
 *     Q = ((cx . P_x) / P_z,  (cy . P_y) / P_z,  1 + (2 . near) / P_z)
 *   in this order of operations; this is where the warped ray through P passes at P.  A point that is not in front (a NaN too) has
 *   Q = (0, 0, 0) and is seen by no view.
 *   Q is rounded to float on store.
 *
 * SEEN.  View u SEES P iff P is in front (ndc != 0 only) and THE LOOKUP of simplenerf_mesh.h succeeds up to, and not including, the
 * depth read: c_z > 0, and the pixel (ix, iy) from rint, ties to even, satisfies 0 <= ix < width and 0 <= iy < height, tested on the
 * floating-point values.  No depth map and no frame is read; views . height . width has no limit here.
 */
#ifndef SIMPLENERF_FIELD_H
#define SIMPLENERF_FIELD_H

#include <stddef.h>

#include "simplenerf_hip.h"
#include "simplenerf_fuse.h"
#include "simplenerf_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_FIELD_NO_VIEW 255        /* snerf_field_point_views: the view byte of a point that no view sees */

/* snerf_field_grid_points: the nodes first_node .. first_node + count - 1 of a grid -> their MLP input points and the number of views
 * that see each.
 *   voxel_size > 0, lo_x, lo_y, lo_z, nx, ny, nz: the grid;  0 <= first_node, first_node + count <= nx . ny . nz
 *   cameras   device (views, SNERF_FUSE_CAMERA_DOUBLES) double;  views 0 .. SNERF_FUSE_MAX_VIEWS, which keeps the count a byte
 *   height, width >= 0: the frame of every view;  ndc, cx, cy, near: THE INPUT MAP
 *   mlp_points device (count, 3) float;  weight  device (count) bytes
 *
 * THE RULE per node: P is its position, mlp_points its Q, weight the number of views, in ascending order, that see P.  views == 0 (or
 * a frame without pixels) gives weight 0 everywhere.  One thread owns one node (one launch).  A block's output equals the same rows
 * of the whole grid's: a caller walks a large grid in blocks and never holds all its points.
 *
 * Errors.  count, first_node, views, height or width negative, first_node + count past the grid, views > SNERF_FUSE_MAX_VIEWS,
 * voxel_size not a finite number > 0, a bound that is not finite, an extent < 1, with ndc != 0 a cx, cy or near that is not finite or
 * near <= 0, or with count > 0 mlp_points or weight NULL, or cameras NULL with views > 0: SNERF_E_INVALID.  A grid above the limit:
 * SNERF_E_UNSUPPORTED.  count == 0 enqueues nothing. */
int snerf_field_grid_points(double voxel_size, double lo_x, double lo_y, double lo_z, int nx, int ny, int nz, long long first_node,
                            long long count, const double* cameras, int views, int height, int width, int ndc, double cx, double cy,
                            double near, float* mlp_points, unsigned char* weight, snerf_stream_t stream);

/* snerf_field_point_views: points of the scene frame -> their MLP input points, and for each the view to look at it from.
 *   points    device (count, 3) float, widened to fp64
 *   cameras, height, width, ndc, cx, cy, near: as above;  views 1 .. SNERF_FUSE_MAX_VIEWS
 *   mlp_points device (count, 3) float;  view_dirs  device (count, 3) float;  view  device (count) bytes
 *
 * THE RULE per point P: mlp_points is its Q.  The CHOSEN view is the one with the smallest c_z among the views that see P, the lowest
 * index among equal ones; view = its index.  If no view sees P, view 0 is used and view = SNERF_FIELD_NO_VIEW.
 *   v_a = P_a - C_a, C the chosen view's centre: the fourth column of the table's inv(E) rows
 *   n = sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2);  dir_a = v_a / n, or (0, 0, 0) when n == 0
 * -- the unit direction of the ray from that camera through P, in the scene frame also when ndc != 0 (a model trained on warped
 * rays still reads the directions of the unwarped ones).  Rounded to float on store.  One thread owns one point (one launch).
 *
 * Errors.  count, height or width negative, views outside 1 .. SNERF_FUSE_MAX_VIEWS, the ndc parameters as above, or with count > 0 a
 * NULL pointer: SNERF_E_INVALID.  count > 2^31 - 1: SNERF_E_UNSUPPORTED.  count == 0 enqueues nothing. */
int snerf_field_point_views(const float* points, long long count, const double* cameras, int views, int height, int width, int ndc,
                            double cx, double cy, double near, float* mlp_points, float* view_dirs, unsigned char* view,
                            snerf_stream_t stream);

/* snerf_field_values: densities -> the signed volume snerf_mesh_count / snerf_mesh_emit take, with `weight` as its weight.
 *   sigma     device (count) float;  weight  device (count) bytes;  level: a finite number > 0, in sigma's units
 *   tsdf      device (count) float
 *
 * THE RULE per element: 1 where weight is 0 or sigma is a NaN; else min(1, max(-1, (level - sigma) / level)) in fp64, rounded to
 * float.  Positive where the density is below the level, 0 at the level, -1 from twice the level up, linear in sigma between: a node
 * is NEGATIVE inside the dense side, so the triangles' normals point out of it.  One thread owns one element (one launch).
 *
 * Errors.  count negative, level not a finite number > 0, or with count > 0 a NULL pointer: SNERF_E_INVALID.  count > 2^31 - 1:
 * SNERF_E_UNSUPPORTED.  count == 0 enqueues nothing. */
int snerf_field_values(const float* sigma, const unsigned char* weight, long long count, double level, float* tsdf,
                       snerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLENERF_FIELD_H */
