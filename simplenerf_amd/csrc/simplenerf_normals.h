/*
 * simplenerf_normals.h -- normal maps in the simplenerf_hip library: the samples of a render that carry weight are selected
 * (snerf_ray_samples_count, snerf_ray_samples_emit), the density field's normals at them are composited along every ray with the
 * render's own weights (snerf_composite_normals), a depth map's normals are formed from its neighbouring pixels' points
 * (snerf_depth_normals), and unit normals become an 8-bit picture (snerf_normals_to_u8).
 * Declared beside include/simplenerf_hip.h like simplenerf_gradient.h (the prototypes of the pinned header groups do not change).
 * Same conventions: status codes, snerf_last_error, device pointers, enqueue-only on `stream`, no allocation, no synchronisation,
 * every check before the first launch.  ABI version 10 is unchanged -- a caller checks that the symbol exists.
 *
 * All device arithmetic is fp64 without fused multiply-adds (fp32 inputs are widened on load) unless a rule says float32; no
 * atomics: every output element has one owning thread, and the same input gives the same bits on every call.
 */
#ifndef SIMPLENERF_NORMALS_H
#define SIMPLENERF_NORMALS_H

#include <stddef.h>

#include "simplenerf_hip.h"
#include "simplenerf_fuse.h"
#include "simplenerf_field.h"
#include "simplenerf_gradient.h"

#ifdef __cplusplus
extern "C" {
#endif

/* snerf_ray_samples_count, snerf_ray_samples_emit: the samples of a render that matter, in order, with the points the MLP saw.
 *   origins, dirs  device (num_rays, 3) float: the rays the render marched (the NDC rays of an NDC render)
 *   z_vals         device (num_rays, num_samples) float: the depths the render sampled
 *   weights        device (num_rays, num_samples) float: the render's compositing weights
 *   min_weight     the threshold, compared in fp64
 *   offsets        device (num_rays + 1) int.  snerf_ray_samples_count writes them; snerf_ray_samples_emit reads them
 *   capacity       the rows of `sample` and `points` (M, read back from offsets[num_rays]); no row at or past it is ever written
 *   sample         device (capacity) int;  points  device (capacity, 3) float
 *
 * THE RULE.  Sample (r, i) is SELECTED iff (double)weights[r, i] > min_weight; a NaN weight is not selected.  offsets[r] is the
 * number of selected samples of the rays before r (an exclusive prefix), offsets[num_rays] = M their total.  The selected samples
 * are numbered in ascending flat index r . num_samples + i; number k has sample[k] = that flat index and
 *   points[k, a] = origins[r, a] + dirs[r, a] * z_vals[r, i]      in FLOAT32: one product, rounded, then one sum
 * -- the expression of the render kernels, so the point is bit for bit the one the MLP was asked at.
 * snerf_ray_samples_count is two launches: a wave per ray counts by ballots, one workgroup scans the counts in place.
 * snerf_ray_samples_emit is one launch: a wave per ray ranks its selected samples by ballots in index order.  A count, a scan and a
 * scatter, as snerf_mesh_count / snerf_mesh_emit; the caller reads M back between the two.
 *
 * Errors.  num_rays or num_samples negative, min_weight a NaN, capacity negative, or a NULL pointer that the call would read or
 * write (offsets always; the others when num_rays . num_samples > 0, the outputs when capacity > 0): SNERF_E_INVALID.
 * num_rays . num_samples > 2^31 - 1: SNERF_E_UNSUPPORTED.  num_rays . num_samples == 0 gives offsets of zeros (num_rays + 1 of them)
 * from snerf_ray_samples_count and enqueues nothing in snerf_ray_samples_emit; so does capacity == 0. */
int snerf_ray_samples_count(const float* weights, long long num_rays, int num_samples, double min_weight, int* offsets,
                            snerf_stream_t stream);
int snerf_ray_samples_emit(const float* origins, const float* dirs, const float* z_vals, const float* weights, long long num_rays,
                           int num_samples, double min_weight, const int* offsets, long long capacity, int* sample, float* points,
                           snerf_stream_t stream);

/* snerf_composite_normals: the field's unit normals at a render's selected samples, composited along every ray.
 *   points         device (count, 3) float: Q, the selected samples' points in the space the MLP reads (snerf_ray_samples_emit)
 *   grad           device (count, 3) float: g, the density's gradient there (snerf_mlp_input_gradient)
 *   offsets, sample  as snerf_ray_samples_emit leaves them;  count = M
 *   weights        device (num_rays, num_samples) float
 *   ndc, cx, cy, near: THE INPUT MAP of simplenerf_field.h
 *   normal         device (num_rays, 3) float;  strength  device (num_rays) float
 *
 * THE RULE per ray r, its selected samples k = offsets[r] .. offsets[r + 1] - 1 in ascending order (a k outside 0 .. count - 1 or
 * a sample[k] outside 0 .. num_rays . num_samples - 1 is skipped: memory outside the buffers is never read):
 *   ndc == 0:  P = Q, G = g.
 *   ndc != 0:  the input map inverted: P_z = (2 . near) / (Q_z - 1), P_x = (Q_x . P_z) / cx, P_y = (Q_y . P_z) / cy.  The sample is
 *     USABLE only if Q_z < 1 and P_z <= -near (a NaN fails both).  G = J^T g at that P, the expression of snerf_field_normals
 *     (simplenerf_gradient.h; one device function serves both).
 *   m = sqrt((G_x G_x + G_y G_y) + G_z G_z).  The sample is usable only if m > 0 and m is finite.  n_a = -G_a / m, kept in fp64.
 *   A_a = A_a + w . n_a over the ray's usable samples, sequentially from 0, w = (double)weights[sample[k]].
 *   s = sqrt((A_x A_x + A_y A_y) + A_z A_z).  normal_a = (float)(A_a / s), strength = (float)s; (0, 0, 0) and 0 where s == 0 or s
 *   is not finite.
 * One thread owns one ray (one launch); a ray's result does not depend on the other rays of the call.
 *
 * Errors.  num_rays, num_samples or count negative, the ndc parameters as in simplenerf_field.h, or with num_rays > 0 a NULL
 * pointer (points, grad and sample may be NULL when count == 0): SNERF_E_INVALID.  num_rays . num_samples or count > 2^31 - 1:
 * SNERF_E_UNSUPPORTED.  num_rays == 0 enqueues nothing. */
int snerf_composite_normals(const float* points, const float* grad, long long count, const int* offsets, const int* sample,
                            const float* weights, long long num_rays, int num_samples, int ndc, double cx, double cy, double near,
                            float* normal, float* strength, snerf_stream_t stream);

/* snerf_depth_normals: the normals of depth maps, from the points of neighbouring pixels.
 *   depth     device (views, height, width) float;  mask  device (views, height, width) bytes, or NULL
 *   cameras   device (views, SNERF_FUSE_CAMERA_DOUBLES) double, the table of simplenerf_fuse.h
 *   edge_threshold  negative: no test
 *   normals   device (views, height, width, 3) float: scene frame, facing the camera
 *
 * THE RULE per pixel (x, y) of view v with depth d.  A pixel is VALID as in simplenerf_fuse.h: d finite and positive, the mask
 * byte (if a mask is given) non-zero.  Its point is the fuse's own, P = inv(E)[:3] [d inv(K) (x, y, 1); 1] (one device function
 * serves both).  A neighbour with depth d' is USABLE iff it lies in the frame, is valid and, with edge_threshold >= 0,
 * |d' - d| <= edge_threshold . d.
 *   t_x = P(x + 1, y) - P(x - 1, y) with both neighbours usable; P(x + 1, y) - P(x, y) with the right one alone; P(x, y) - P(x - 1, y)
 *         with the left one alone; none with neither.
 *   t_y likewise from (x, y - 1) above and (x, y + 1) below: P(below) - P(above), P(below) - P, P - P(above).
 *   c = t_x x t_y, every component two products and one subtraction: c_x = t_x,y t_y,z - t_x,z t_y,y; c_y = t_x,z t_y,x - t_x,x t_y,z;
 *   c_z = t_x,x t_y,y - t_x,y t_y,x.  m = sqrt((c_x c_x + c_y c_y) + c_z c_z).
 *   n = c / m, negated if (n_x (C_x - P_x) + n_y (C_y - P_y)) + n_z (C_z - P_z) < 0, with C the view's centre (column 3 of inv(E)).
 *   (0, 0, 0) for a pixel that is not valid, a missing tangent, or m == 0 or not finite.  Rounded to float on store.
 * One thread owns one pixel (one launch).
 *
 * Errors.  views, height or width negative, views > SNERF_FUSE_MAX_VIEWS, edge_threshold a NaN, or with views . height . width > 0
 * a NULL depth, cameras or normals: SNERF_E_INVALID.  views . height . width > 2^31 - 1: SNERF_E_UNSUPPORTED.  No pixel: nothing is
 * enqueued. */
int snerf_depth_normals(const float* depth, const unsigned char* mask, const double* cameras, int views, int height, int width,
                        double edge_threshold, float* normals, snerf_stream_t stream);

/* snerf_normals_to_u8: unit normals as a picture.
 *   normals   device (count, 3) float
 *   rotation  HOST array of 9 doubles, a row-major 3x3 matrix R (a camera-to-world rotation), or NULL for the identity
 *   image     device (count, 3) bytes
 *
 * THE RULE per normal n: c_a = (R[0][a] n_0 + R[1][a] n_1) + R[2][a] n_2 (c = R^T n: the normal in the camera's frame);
 * u8_a = min(255, max(0, floor(127.5 . (c_a + 1) + 0.5))); a NaN gives 0 -- so a normal with a NaN component is (0, 0, 0),
 * since every c_a holds a product with it, and an infinite component leaves the other two 0 (0 . inf).  A zero normal is (128, 128, 128); with a camera looking
 * down -z, y up, a surface facing the camera comes out blue.
 * One thread owns one normal (one launch).
 *
 * Errors.  count negative, an entry of R that is not finite, or with count > 0 a NULL normals or image: SNERF_E_INVALID.
 * count > 2^31 - 1: SNERF_E_UNSUPPORTED.  count == 0 enqueues nothing. */
int snerf_normals_to_u8(const float* normals, long long count, const double* rotation, unsigned char* image, snerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLENERF_NORMALS_H */
