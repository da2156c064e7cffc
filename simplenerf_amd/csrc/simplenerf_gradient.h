/*
 * simplenerf_gradient.h -- the gradient of a model's density field with respect to the point it is asked at, in the simplenerf_hip
 * library: snerf_mlp_input_gradient runs the fp32 backward chain of snerf_mlp_backward without its weight-gradient launches and
 * carries dY_0 (and, through the skip connection, dY_5) on through the first layer's weights and the positional encoding's Jacobian;
 * snerf_field_normals pulls that gradient back through THE INPUT MAP of simplenerf_field.h and writes unit outward normals.
 * Declared beside include/simplenerf_hip.h like simplenerf_field.h (the prototypes of the pinned header groups do not change).  Same
 * conventions: status codes, snerf_last_error, device pointers, enqueue-only on `stream`, no allocation, no synchronisation, every
 * check before the first launch.  ABI version 10 is unchanged -- a caller checks that the symbol exists.
 */
#ifndef SIMPLENERF_GRADIENT_H
#define SIMPLENERF_GRADIENT_H

#include <stddef.h>

#include "simplenerf_hip.h"
#include "simplenerf_field.h"

#ifdef __cplusplus
extern "C" {
#endif

/* snerf_mlp_input_gradient: d_points[i, :] = d_sigma[i] . d sigma_i / d x_i for num_points points x_i, each a ray of ONE sample.
 *   desc, packed  the MLP and its weight stream from snerf_mlp_pack_for(SNERF_PRECISION_FP32, training = 1) (or snerf_mlp_pack)
 *   params        host array of num_params device pointers, the reference-layout tensors that were packed, in the order of
 *                 snerf_mlp_pack: pts_linears.0.weight (width, pts_in) and, when points_net_depth > 5, pts_linears.5.weight
 *                 (width, pts_in + width) are read; num_params = snerf_mlp_num_params(desc)
 *   saved_acts, sigma   what snerf_mlp_forward_train(desc, packed, origins = the points, dirs = 0, view_dirs, depths = 0,
 *                 num_rays = num_points, num_samples = 1, sigma_noise = NULL, ..., SNERF_PRECISION_FP32) wrote for these points
 *   d_sigma       device (num_points) float: the factor per point (1 for the plain gradient)
 *   workspace     device, snerf_mlp_input_gradient_workspace_floats(desc, num_points) floats; contents undefined afterwards
 *   d_points      device (num_points, 3) float
 *
 * THE RULE.  The chain of snerf_mlp_backward runs with d_rgb = 0, so the colour branch adds exact zeros and every dY_l is that of
 * sigma alone.  With pts_in the number of encoding features the trunk reads (3 + 6 . points_pe_degree, or 3 + 6 .
 * sigma_pe_degree for the points-augmentation layout: the gradient covers what the trunk reads),
 *   d enc = W_0^T dY_0 (+ W_5[:, :pts_in]^T dY_5 when points_net_depth > 5)      fp32 matrix cores, a fixed order of sums
 *   d x_a = d enc_a + sum_k 2^k (cos(2^k x_a) . d sin_{k,a} - sin(2^k x_a) . d cos_{k,a})      a = 0, 1, 2;  k = 0 .. degree - 1
 * where sin(2^k x_a) and cos(2^k x_a) are the encoding rows the forward saved and the sum over the encoding features is formed in
 * fp64 in ascending feature order per half of the features, the two halves added last; rounded to float on store.  One thread owns
 * one output element, no atomics: the same input gives the same bits on every call, and a point's gradient does not depend on
 * which other points are in the call.  A point with sigma == 0 (the density's ReLU is closed) has d_points = (+0, +0, +0).
 *
 * Limits.  SNERF_PRECISION_FP32 only -- only the fp32 chain keeps fp32 dY tiles --, the fused shapes only (width 256 with views
 * width 128, width 128 with views width 64, or either width without a views layer), no predict_visibility.
 *
 * Errors.  A NULL pointer, num_points < 1, num_params not snerf_mlp_num_params(desc), a packed buffer whose last pack did not write
 * the fp32 streams (one packed for a 16-bit precision only): SNERF_E_INVALID.  A shape of the layered path, a predict_visibility descriptor, more than 2^31 - 1
 * 128-sample workgroups: SNERF_E_UNSUPPORTED.  Nothing is enqueued then.
 * snerf_mlp_input_gradient_workspace_floats returns 0 for a descriptor or count the call would refuse. */
size_t snerf_mlp_input_gradient_workspace_floats(const snerf_mlp_desc* desc, long long num_points);

int snerf_mlp_input_gradient(const snerf_mlp_desc* desc, const float* packed, const float* const* params, int num_params,
                             const float* saved_acts, const float* sigma, const float* d_sigma, long long num_points,
                             float* workspace, float* d_points, snerf_stream_t stream);

/* snerf_field_normals: the gradient of the density in the MLP's input space -> unit outward normals in the scene frame.
 *   points_scene  device (count, 3) float: the points P in the scene frame (the mesh's vertices), widened to fp64
 *   grad_mlp      device (count, 3) float: g = the density's gradient at Q(P), in the space the MLP reads (snerf_mlp_input_gradient)
 *   ndc, cx, cy, near: THE INPUT MAP of simplenerf_field.h
 *   normals       device (count, 3) float
 *
 * THE RULE per point, in fp64 without fused multiply-adds:
 *   ndc == 0:  G = g.
 *   ndc != 0:  G = J^T g with J the Jacobian of Q = ((cx . P_x) / P_z, (cy . P_y) / P_z, 1 + (2 . near) / P_z):
 *     G_x = (cx / P_z) . g_x
 *     G_y = (cy / P_z) . g_y
 *     G_z = -(((cx . P_x) . g_x + (cy . P_y) . g_y) + (2 . near) . g_z) / (P_z . P_z)
 *   m = sqrt((G_x G_x + G_y G_y) + G_z G_z);  n_a = -G_a / m, rounded to float.  The density's low side is outside: the sign of
 *   snerf_field_values and the winding of the mesh.
 *   (0, 0, 0) where m == 0 or m is not finite, and with ndc != 0 where P is not IN FRONT (P_z <= -near fails; a NaN too).
 * One thread owns one point (one launch); no atomics; the same bits on every call.
 *
 * Errors.  count negative, the ndc parameters as in simplenerf_field.h, or with count > 0 a NULL pointer: SNERF_E_INVALID.
 * count > 2^31 - 1: SNERF_E_UNSUPPORTED.  count == 0 enqueues nothing. */
int snerf_field_normals(const float* points_scene, const float* grad_mlp, long long count, int ndc, double cx, double cy, double near,
                        float* normals, snerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLENERF_GRADIENT_H */
