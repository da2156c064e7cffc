/*
 * simplenerf_sweep.h -- the view sweep of the simplenerf_hip library, declared beside include/simplenerf_hip.h instead of in it
 * (the prototypes of the two headers under include/ are a pinned set, and so is the group of simplenerf_maps.h).  Same conventions
 * (status codes, snerf_last_error, device pointers, `stream`); ABI version 10 is unchanged -- no existing struct or signature
 * changed, a caller checks that the symbols exist.
 */
#ifndef SIMPLENERF_SWEEP_H
#define SIMPLENERF_SWEEP_H

#include "simplenerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One rendered pose under the view directions of many other cameras (the reference's start_testing_static_videos: rays of
 * extrinsics[0], view directions of every camera of the spiral path).  With the rays fixed and no draws, everything of a render
 * up to the views layer's pre-activation is shared by all V views; per view only
 *     u[v,n,j]     = b_v[j] + sum_e W_v[j, W+e] * PE(d[v,n])[e]         (27 terms at degree 4, e ascending)
 *     g[n,s,j]     =          sum_i W_v[j, i]   * feature[n,s,i]         (once for all views; fp32 matrix cores, i ascending)
 *     rgb[v,n,s,c] = sigmoid(b_o[c] + sum_j W_o[c,j] * relu(g[n,s,j] + u[v,n,j]))
 *     out[v,n,c]   = sum_s weights[n,s] * rgb[v,n,s,c]   (+ 1 - acc[n] when white_bkgd)
 * differs.  W_v = views_linears.0.weight (Wv x (W+27)), W_o = views_output_linear.weight (3 x Wv), PE in the reference's order.
 *   desc, params   as snerf_mlp_pack takes them (host array of device pointers, C-ABI parameter order).  The weights are read from
 *                  the parameter tensors, not from a packed stream: of the five tensors the sweep reads (W_v's feature columns,
 *                  its encoding columns, b_v, W_o, b_o) the fp32 stream holds only the first in an order a matrix-core loop
 *                  can use, so one transposing launch (128 KB) buys a single source in natural order and independence from
 *                  what a buffer was last packed for.
 *   saved_acts     what snerf_mlp_forward_train / a keep_activations render wrote for these (num_rays, num_samples) at
 *                  SNERF_PRECISION_FP32 (snerf_mlp_saved_floats floats): the `feature` tile of every 32-sample block is read
 *   weights, acc   (n,S), (n) of the compositing; acc may be NULL unless white_bkgd
 *   view_dirs      (V,n,3) unit view directions;  out_rgb  (V,n,3)
 *   workspace      device scratch of at least the query below, 16-byte aligned; no initial state, calls enqueued on ONE stream may
 *                  share it
 * All arithmetic is fp32.  The sum over s runs s = 0 .. S-1 in one thread per (view, ray, channel): no atomics, two calls give the
 * same bits, out[v] depends neither on V nor on the other views of the call, and a ray's result does not depend on where its
 * samples fall in the 32-sample blocks.
 * Built for the view-dependent layouts of the fused fp32 kernels, (points_net_width, views_net_width) = (256, 128) and (128, 64),
 * with sigma_pe_degree = -1 and predict_visibility = 0; anything else is SNERF_E_UNSUPPORTED with a message (the workspace query
 * then returns 0).  A NULL descriptor, a negative count and num_samples < 1 are SNERF_E_INVALID; num_rays == 0 or num_views == 0
 * then enqueues nothing and returns SNERF_OK; in any other call a NULL pointer, num_params other than the descriptor's and
 * white_bkgd without acc are SNERF_E_INVALID.  Every check happens before the first launch.  Only enqueues on `stream` (four
 * launches): no allocation, no synchronisation. */
size_t snerf_view_sweep_workspace_floats(const snerf_mlp_desc* desc, long long num_rays, int num_samples, int num_views);
int snerf_view_sweep(const snerf_mlp_desc* desc, const float* const* params, int num_params, const float* saved_acts,
                     const float* weights, const float* acc, const float* view_dirs, long long num_rays, int num_samples,
                     int num_views, int white_bkgd, float* out_rgb, float* workspace, snerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLENERF_SWEEP_H */
