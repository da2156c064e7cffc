/*
 * simplenerf_sweep16.h -- the view sweep from the 16-bit saved activations (SNERF_PRECISION_F16 / _BF16), declared beside
 * simplenerf_sweep.h instead of in it: that header's prototypes are a pinned set, like those of the two headers under include/ and
 * of simplenerf_maps.h.  Same conventions (status codes, snerf_last_error, device pointers, `stream`); ABI version 10 is unchanged
 * -- no existing struct or signature changed, a caller checks that the symbols exist.
 */
#ifndef SIMPLENERF_SWEEP16_H
#define SIMPLENERF_SWEEP16_H

#include "simplenerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* snerf_view_sweep (simplenerf_sweep.h: one rendered pose under the view directions of V other cameras) for a model that renders
 * at SNERF_PRECISION_F16 or SNERF_PRECISION_BF16.  The formula is that header's, on the operands the 16-bit render itself
 * multiplies; r() rounds an fp32 value to the mode's 16-bit format, to nearest even (what snerf_mlp_pack does to the weights of
 * the mode's stream and the 16-bit kernels do to their activations):
 *     u[v,n,j]     = b_v[j] + sum_e r(W_v[j, W+e]) * r(PE(d[v,n])[e])     (fp32 sum, e ascending; the products are exact in fp32)
 *     g[n,s,j]     =          sum_i r(W_v[j, i])   * feature16[n,s,i]      (once for all views: v_mfma_f32_32x32x16_f16 / _bf16,
 *                                                                           fp32 accumulation, 16 features per instruction)
 *     rgb[v,n,s,c] = sigmoid(b_o[c] + sum_j W_o[c,j] * relu(g[n,s,j] + u[v,n,j]))            (fp32, as the 16-bit kernels' heads)
 *     out[v,n,c]   = sum_s weights[n,s] * rgb[v,n,s,c]   (+ 1 - acc[n] when white_bkgd)       (fp32, s ascending)
 * u and g differ from the views layer of the mode's own render in the order of their fp32 sums only.
 *   desc, params   as snerf_view_sweep takes them: the weights are read from the parameter tensors and rounded here (one launch
 *                  writes r(W_v[:, :W]) into the workspace in matrix-core operand order), not from a packed stream
 *   saved_acts     what snerf_mlp_forward_train / a keep_activations render wrote for these (num_rays, num_samples) at `precision`
 *                  (SNERF_PRECISION_F16S8 / _BF16S8 keep `feature` like their base mode: pass the base mode).  Read: the
 *                  `feature` pieces of every 32-sample block, the first snerf_view_sweep_half_acts_floats floats at most.
 *   precision      SNERF_PRECISION_F16 or SNERF_PRECISION_BF16: the format of the pieces and of r()
 *   weights, acc, view_dirs, out_rgb, workspace, stream      as in snerf_view_sweep (workspace: the query below, 16-byte aligned)
 *
 * The `feature` pieces.  In the 16-bit modes the saved activations are rows of 32 x 16 bit (64 bytes).  The sample blocks are
 * 32 consecutive samples of the (num_rays x num_samples) sequence; block b starts at row b * R, R = 96 + (D + 1) W + Wv +
 * 4 * ceil((D W / 32 + Wv / 32) / 2) (D = points_net_depth, W = points_net_width, Wv = views_net_width), and its `feature` tensor
 * at row 96 + D W of the block, W rows long: W / 16 "pieces" of 1 KiB (16 rows), piece k holding features 16 k .. 16 k + 15 of the
 * block's 32 samples.  A piece is the image of a matrix-core operand: 64 slots of 16 bytes, slot 2 j + h of lane (j = lane & 31,
 * h = lane >> 5); the lane's eight 16-bit elements e = 0 .. 7 are
 *     feature 16 k + 8 (e >> 2) + 4 h + (e & 3)   of sample j of the block
 * -- so sample j owns the 32 consecutive bytes 32 j .. 32 j + 31 of the piece, with its features 16 k + {0 1 2 3, 8 9 10 11} in the
 * first 16 and 16 k + {4 5 6 7, 12 13 14 15} in the second 16.  Read as it lies, a lane's slot is its B operand of k-step k: lane
 * half h supplies the k-indices 8 h + e of the instruction, and the A operand written into the workspace holds r(W_v[32 t + j,
 * 16 k + 8 (e >> 2) + 4 h + (e & 3)]) in element e of lane (j, h) for out tile t: the same feature under the same k-index.  Samples
 * past num_rays * num_samples in the last block hold finite values nobody uses.
 *
 * All guarantees of snerf_view_sweep hold: the sum over s runs s = 0 .. S-1 in one thread per (view, ray, channel), no atomics, two
 * calls give the same bits, out[v] depends neither on V nor on the other views of the call, and a ray's result does not depend on
 * where its samples fall in the 32-sample blocks.  No fp16 range handling: the features were range-checked by the forward that
 * wrote them, and a weight outside the fp16 range already fails at snerf_mlp_pack.
 * Built for the view-dependent layouts the 16-bit storing forward and snerf_view_sweep share, (points_net_width, views_net_width) =
 * (256, 128) and (128, 64), with sigma_pe_degree = -1 and predict_visibility = 0; anything else is SNERF_E_UNSUPPORTED with a
 * message (the two queries then return 0).  A NULL descriptor, a negative count, num_samples < 1 and a `precision` other than the
 * two above are SNERF_E_INVALID (fp32 activations: snerf_view_sweep); num_rays == 0 or num_views == 0 then enqueues nothing and
 * returns SNERF_OK; in any other call a NULL pointer, num_params other than the descriptor's and white_bkgd without acc are
 * SNERF_E_INVALID.  Every check happens before the first launch.  Only enqueues on `stream` (four launches): no allocation, no
 * synchronisation. */
size_t snerf_view_sweep_half_workspace_floats(const snerf_mlp_desc* desc, long long num_rays, int num_samples, int num_views);
size_t snerf_view_sweep_half_acts_floats(const snerf_mlp_desc* desc, long long num_rays, int num_samples);
int snerf_view_sweep_half(const snerf_mlp_desc* desc, const float* const* params, int num_params, const float* saved_acts,
                          const float* weights, const float* acc, const float* view_dirs, long long num_rays, int num_samples,
                          int num_views, int white_bkgd, int precision, float* out_rgb, float* workspace, snerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLENERF_SWEEP16_H */
