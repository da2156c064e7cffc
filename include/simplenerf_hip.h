/*
 * simplenerf_hip.h -- C ABI of the MI355X (gfx950) volumetric renderer for SimpleNeRF's ray-marching path.
 *
 * Drop-in boundary: every entry point replaces one function of the reference's Python path (file:line below are
 * relative to the reference checkout).  All pointers marked "device" are HIP device pointers to contiguous fp32
 * arrays in the reference's row-major layouts; `stream` is a hipStream_t passed as void* (NULL = default stream).
 * Calls only enqueue work on `stream`; they never synchronise, allocate or free (safe under hipGraph capture).
 *
 * Return value: 0 on success, negative snerf_status on failure; snerf_last_error() returns a thread-local
 * message for the last failure on the calling thread.  There is no CPU fallback: without a HIP device every
 * compute entry point fails with SNERF_E_HIP.
 */
#ifndef SIMPLENERF_HIP_H
#define SIMPLENERF_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* snerf_stream_t; /* hipStream_t */

enum snerf_status {
    SNERF_OK = 0,
    SNERF_E_INVALID = -1,     /* bad argument (null pointer, non-positive size, ...) */
    SNERF_E_UNSUPPORTED = -2, /* configuration outside what the kernels are built for */
    SNERF_E_HIP = -3,         /* HIP runtime error (message carries hipGetErrorString) */
    SNERF_E_RANGE = -4        /* an EARLIER fp16-mode launch on this device met a value outside the fp16 range (see
                                 snerf_range_status): its results are wrong; reported once by the next fp16-mode call */
};

/* ABI version of this header; bumped on any signature change (new enum values such as SNERF_PRECISION_F16 extend a
 * version without changing it: older callers never pass them). */
#define SNERF_ABI_VERSION 10
/* Threads (no ABI change): every entry point may be called from several host threads at once -- on different devices, on
 * different streams of one device, and on the SAME stream (torch.nn.DataParallel with a repeated device id runs its replicas in
 * parallel threads that enqueue on one stream).  The host-side state the library keeps is guarded: ONE table holds one state per
 * (device, stream) -- its enqueue lock, the side streams and fork / join events of the render calls, the layered path's inference
 * scratch blocks -- and a render call (snerf_render_forward / _backward) or a layered-shape snerf_mlp_forward holds that lock from
 * its first launch to its join, so two calls on one stream enqueue one after the other, never interleaved, and nothing else in
 * the state needs a lock of its own; the packed-format registry, the timing table and the range table sit behind mutexes; kernel
 * attributes and the CU count are settled once per device with atomic flags; the error message is thread-local.  What the caller owns stays the caller's: two threads must not write the same output or
 * workspace buffers, or re-pack a weight buffer another thread's call still reads.  The fp16 range flag is one per DEVICE:
 * the next fp16-mode call on that device reports it, from whichever thread. */
int snerf_abi_version(void);
const char* snerf_last_error(void);

/* ---------------------------------------------------------------------------------------------------------------
 * K1  ray generation.  Replaces DataPreprocessor.get_rays (src/data_preprocessors/DataPreprocessor01.py:351-368),
 * get_view_dirs (:392-394) and get_ndc_rays (:371-389) for the pixel range [first_ray, first_ray+num_rays) of an
 * height x width frame (row-major pixel index, x fastest), so that each rank of a sharded render generates only
 * its own rays.
 *   intrinsic   host, 3x3 row-major        pose  host, 4x4 row-major *processed* camera-to-world (the matrix
 *               the reference hands to get_rays; see create_test_data :816-831)
 *   pixel_offset  0 (reference default) or 0.5 (its 'mip_nerf' switch, :357-359)
 *   near        world near plane used by the NDC warp (model_configs['near'])
 *   outputs     device, (num_rays,3) each; rays_o_ndc / rays_d_ndc may be NULL when ndc == 0; view_dirs may be NULL
 */
int snerf_generate_rays(int height, int width, const float* intrinsic, const float* pose, float pixel_offset,
                        int ndc, float near, long long first_ray, long long num_rays, float* rays_o, float* rays_d,
                        float* view_dirs, float* rays_o_ndc, float* rays_d_ndc, snerf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K2  coarse depths.  Replaces SimpleNeRF.get_z_vals_coarse (src/models/SimpleNeRF01.py:272-302).
 *   near, far   device (num_rays)           t_rand  device (num_rays, num_samples) uniform [0,1) draws for the
 *               stratified jitter of :293-301, or NULL for the unperturbed (eval) depths
 *   depths      device (num_rays, num_samples)
 */
int snerf_coarse_depths(const float* near, const float* far, long long num_rays, int num_samples, int lindisp,
                        const float* t_rand, float* depths, snerf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K3  positional encoding + MLP.  Replaces run_network/batchify + MLP.forward (src/models/SimpleNeRF01.py:363-428,
 * :560-715) including the sample-position computation of render_rays (:139-142, :203-206).
 */
typedef struct snerf_mlp_desc {
    int points_net_depth;    /* number of trunk Linear layers (skip re-injection after layer index 4, :580) */
    int points_net_width;    /* 128 or 256 */
    int views_net_depth;     /* 1 (only value any shipped config uses) when view_dependent_rgb, else ignored */
    int views_net_width;     /* 64 or 128 */
    int points_pe_degree;    /* <= 10 */
    int views_pe_degree;     /* <= 4; ignored unless use_view_dirs */
    int sigma_pe_degree;     /* points_sigma_positional_encoding_degree (:576-578), or -1 when the key is absent */
    int use_view_dirs;
    int view_dependent_rgb;
    int predict_visibility;  /* :582-584, :599-602: views_output_linear gets a 4th row, the per-sample visibility of the point
                                from a view direction (sigmoid).  Built for view_dependent_rgb MLPs, fp32 arithmetic; off in
                                every shipped configuration */
} snerf_mlp_desc;

/* Number of entries of the `params` array below for this descriptor (0 if unsupported):
 *   [2i], [2i+1]  pts_linears.i.weight (out,in), .bias           i = 0 .. points_net_depth-1
 *   then          pts_output_linear.weight, .bias
 *   then, if view_dependent_rgb: feature_linear.weight, .bias; views_linears.0.weight, .bias;
 *                 views_output_linear.weight, .bias
 * i.e. the reference state_dict tensors (MLP.__init__ :586-608), each a device pointer. */
int snerf_mlp_num_params(const snerf_mlp_desc* desc);

/* Size in floats of the packed (MFMA-operand-ordered) weight stream; 0 if the descriptor is unsupported. */
size_t snerf_mlp_packed_floats(const snerf_mlp_desc* desc);

/* Re-order the reference-layout parameters into the packed stream (device -> device).  Call after every
 * parameter update; the stream is what snerf_mlp_forward consumes. */
int snerf_mlp_pack(const snerf_mlp_desc* desc, const float* const* params, int num_params, float* packed,
                   snerf_stream_t stream);

/* snerf_mlp_pack writes EVERY operand format of the weights (fp32 segments, the fp16 hi/lo streams for training and for
 * rendering, their bf16 counterparts): a trainer that re-packs after every optimiser step pays for seven of them and reads
 * two (the fp32 precision: the fp32 segments alone).  This variant writes what calls at ONE precision (enum snerf_precision, below) in ONE mode will read -- training != 0:
 * snerf_mlp_forward_train / snerf_mlp_backward / the render ops with saved activations; training == 0: additionally the
 * rendering layout -- and zeroes the rest: the caller re-packs when it changes precision or mode (the Python model keys its
 * packed streams by both).  No counterpart in the reference (its modules read their parameters directly).
 *
 * Round 5: the library remembers, per packed buffer (by address, host side), which formats its last pack call wrote, and every
 * entry point that reads a weight stream (snerf_mlp_forward[_train|_visibility], snerf_mlp_backward, the render calls) returns
 * SNERF_E_INVALID before enqueuing anything when the buffer does not hold what the call reads -- a stream packed for (f16,
 * training) used by an eval render used to multiply the zero-filled rendering layout and return bias-only output with SNERF_OK.
 * A buffer no pack call of this library instance has written (a device-to-device copy of a packed buffer) is not checked. */
int snerf_mlp_pack_for(const snerf_mlp_desc* desc, const float* const* params, int num_params, float* packed, int precision,
                       int training, snerf_stream_t stream);

enum snerf_precision {
    SNERF_PRECISION_FP32 = 0, /* fp32 MFMA (v_mfma_f32_32x32x2_f32), exact fp32 FMA chains */
    SNERF_PRECISION_F16X3 = 1, /* every operand split into two fp16 (hi + lo, ~22 significand bits), three fp16 MFMAs per
                                  product (hi.hi + hi.lo + lo.hi), fp32 accumulate: fp32-grade results at 3/16 of the
                                  fp32-MFMA time */
    SNERF_PRECISION_F16 = 2,   /* 16-bit mode: one fp16 MFMA per product (11 significand bits per operand), fp32 accumulate,
                                  fp32 master weights, biases, heads and outputs; training keeps activations as fp16 and
                                  layer gradients as bf16 (half the HBM traffic).  NOT within the fp32 parity bar: results
                                  agree with the fp32 path to ~1e-3 (tests/test_gpu_f16.py states the tolerances) */
    SNERF_PRECISION_F16S8 = 4, /* SNERF_PRECISION_F16 with the saved trunk activations h_1 .. h_D-1 kept as fp8 e4m3 (half their bytes
                                  on the way out and back in): they are read back only as the X operand of the weight-gradient
                                  contraction over ~10^6 samples, where a 2^-4 rounding error per element averages out; values above
                                  448 are clamped there.  Rendering, the training forward's arithmetic and the backward chain are
                                  SNERF_PRECISION_F16's; only the weight gradients differ (<= 1e-2 relative L2,
                                  tests/test_gpu_f16.py) */
    SNERF_PRECISION_BF16S8 = 5, /* SNERF_PRECISION_BF16 with the saved trunk activations as fp8 e4m3, as SNERF_PRECISION_F16S8 is to
                                   SNERF_PRECISION_F16: BASELINE config 5's literal dtype with 15 % fewer HBM bytes per iteration */
    SNERF_PRECISION_BF16 = 3   /* the same kernels on bf16 operands (v_mfma_f32_*_bf16, 8 significand bits, fp32's exponent
                                  range): BASELINE config 5's literal dtype.  No range limit -- nothing below under "Range"
                                  applies -- at 3 fewer significand bits than SNERF_PRECISION_F16; saved activations and layer
                                  gradients both bf16.  Own tolerances (tests/test_gpu_bf16.py).  Also built for every MLP
                                  shape of the layered path (mlp_generic_bf16.hip), where SNERF_PRECISION_BF16S8 is this mode
                                  bit for bit; the fp16 modes are refused for those shapes */
};
/* Range: both fp16 modes hold hidden activations and weights as fp16 numbers (pairs), so their magnitudes must stay
 * below 65504 -- far above what a NeRF MLP on encoded inputs produces (trained hidden units are O(1..100)).  Exceeding it
 * is DETECTED, not silent: an operand beyond the range converts to +-inf, which makes every pre-activation of the next layer
 * non-finite for that sample, so every fp16-mode forward kernel checks one pre-activation per sample and layer before its
 * ReLU could mask it (one instruction per layer; csrc/mlp_device_f16.h, RangeWatch), and snerf_mlp_pack checks the weights;
 * a launch that met a non-finite operand raises a per-device flag in pinned host memory when it finishes.  Launches are asynchronous, so the
 * flag is reported like an asynchronous HIP error: the NEXT fp16-mode call on that device (snerf_mlp_forward[_train],
 * snerf_mlp_backward, the render ops) fails with SNERF_E_RANGE before enqueuing anything and clears it; after a
 * synchronisation snerf_range_status tells at once.  Outputs of a flagged launch must be discarded (an overflowed unit can
 * be masked by a later ReLU, so they may look finite).  Gradients have no such limit (renormalised by powers of two).  The
 * fp32 mode has the full fp32 range and never raises the flag.
 *   snerf_range_status(clear)   bit 0: an activation / encoded input left the fp16 range; bit 1: a weight did (set by
 *                               snerf_mlp_pack, which cannot know the precision it packs for: only fp16-mode calls report it);
 *                               0 = clean; < 0 = error.  `clear` != 0 resets the flag of the current device.
 * The first fp16-mode call (or snerf_mlp_pack) of a process allocates the 256-byte flag table with hipHostMalloc: make it
 * outside of a graph capture. */
int snerf_range_status(int clear);

/*   origins, dirs   device (num_rays,3): the rays the depths are measured along (NDC rays when ndc)
 *   view_dirs       device (num_rays,3) or NULL when !use_view_dirs
 *   depths          device (num_rays, num_samples)
 *   sigma_noise     device (num_rays, num_samples) added to the raw density before the ReLU (:669-672), or NULL
 *   sigma           device (num_rays, num_samples)      = 'sigma' of MLP.forward, post-ReLU
 *   rgb             device (num_rays, num_samples, 3)   = 'rgb' of MLP.forward, post-sigmoid
 */
int snerf_mlp_forward(const snerf_mlp_desc* desc, const float* packed, const float* origins, const float* dirs,
                      const float* view_dirs, const float* depths, long long num_rays, int num_samples,
                      const float* sigma_noise, float* sigma, float* rgb, int precision, snerf_stream_t stream);

/* ---- training: forward that keeps the per-layer activations, and the parameter-gradient backward (K7) -----------
 * Together they replace what autograd records and replays for MLP.forward (src/models/SimpleNeRF01.py:626-715).
 *   saved_acts   device, snerf_mlp_saved_floats(desc, num_rays, num_samples) floats, written by forward_train and
 *                read by backward ([32-sample block][feature][32] tiles: encodings and every layer's input)
 *   d_sigma (n,S), d_rgb (n,S,3)   device: gradients w.r.t. the `sigma` / `rgb` outputs of the forward
 *   sigma, rgb                      device: those outputs themselves (ReLU / sigmoid derivatives)
 *   workspace    device, snerf_mlp_backward_workspace_floats(...) floats of scratch
 *   param_grads  num_params device pointers, same order and shapes as snerf_mlp_pack's `params`; each tensor is
 *                OVERWRITTEN with dL/dparam when accumulate == 0, or has dL/dparam ADDED to it when accumulate != 0
 *                (what autograd does with the gradients of the trainer's second sub-batch, src/Trainer01.py:82-96, without
 *                a separate add launch per tensor).  Sums over samples are taken in a fixed order: bit-reproducible
 *   precision    SNERF_PRECISION_FP32; SNERF_PRECISION_F16X3 for the fp16-split forward_train / dgrad chain / large
 *                weight-gradient products (the small head and encoding products stay on the fp32 matrix cores); or
 *                SNERF_PRECISION_F16 (16-bit mode).  MLP shapes outside the fused kernels' set (the layered path) take
 *                SNERF_PRECISION_FP32, SNERF_PRECISION_BF16 and SNERF_PRECISION_BF16S8 (= BF16 there) and refuse the
 *                fp16 modes.  The layout of saved_acts depends on the precision: pass to
 *                snerf_mlp_backward the precision that snerf_mlp_forward_train was called with (both buffer-size
 *                queries are valid for every precision)
 * Inputs (rays, depths, view directions) receive no gradient -- the reference detaches the sample depths (:312).
 */
size_t snerf_mlp_saved_floats(const snerf_mlp_desc* desc, long long num_rays, int num_samples);
int snerf_mlp_forward_train(const snerf_mlp_desc* desc, const float* packed, const float* origins, const float* dirs,
                            const float* view_dirs, const float* depths, long long num_rays, int num_samples,
                            const float* sigma_noise, float* sigma, float* rgb, float* saved_acts, int precision,
                            snerf_stream_t stream);
size_t snerf_mlp_backward_workspace_floats(const snerf_mlp_desc* desc, long long num_rays, int num_samples);
int snerf_mlp_backward(const snerf_mlp_desc* desc, const float* packed, const float* saved_acts, const float* sigma,
                       const float* rgb, const float* d_sigma, const float* d_rgb, long long num_rays, int num_samples,
                       float* workspace, float* const* param_grads, int num_params, int precision, int accumulate,
                       snerf_stream_t stream);

/* ---- predict_visibility (src/models/SimpleNeRF01.py:317-326, :646-649, :691-714, :479-482) -----------------------------
 * snerf_other_view_dirs: SimpleNeRF.compute_other_view_dirs -- unit directions from each of `num_other` secondary camera
 * centres to every sample point, (n, S, num_other, 3).  With ndc the sample depths are converted to world depths first
 * (near plane hard-coded to 1 as in the reference, :319-321).
 *   depths (n,S); rays_o, rays_d (n,3) WORLD rays; rays_o2 (n, num_other, 3)
 * snerf_mlp_forward_visibility: snerf_mlp_forward[_train] for a predict_visibility MLP; additionally
 *   visibility   (n,S)             'visibility' of MLP.forward for the primary view direction, or NULL
 *   view_dirs2   (n,S,num_other,3) per-sample secondary directions (snerf_other_view_dirs), or NULL with num_other = 0
 *   visibility2  (n,S,num_other)   'visibility2': the views head evaluated again per secondary direction (:646-649)
 *   saved_acts   NULL for inference; else as snerf_mlp_forward_train (the visibility outputs carry no gradient: no shipped
 *                loss reads them, and snerf_mlp_backward writes zeros for the 4th row of views_output_linear)
 * snerf_composite_visibility2: 'visibility2' of volume_rendering (:479-482): sum_s w[n,s] vis2[n,s,k] / (acc[n] + 1e-6).
 */
int snerf_other_view_dirs(const float* depths, const float* rays_o, const float* rays_d, const float* rays_o2,
                          long long num_rays, int num_samples, int num_other, int ndc, float* view_dirs2,
                          snerf_stream_t stream);
int snerf_mlp_forward_visibility(const snerf_mlp_desc* desc, const float* packed, const float* origins, const float* dirs,
                                 const float* view_dirs, const float* depths, long long num_rays, int num_samples,
                                 const float* sigma_noise, const float* view_dirs2, int num_other, float* sigma, float* rgb,
                                 float* visibility, float* visibility2, float* saved_acts, int precision,
                                 snerf_stream_t stream);
int snerf_composite_visibility2(const float* weights, const float* acc, const float* visibility2, long long num_rays,
                                int num_samples, int num_other, float* out, snerf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K4  alpha compositing.  Replaces SimpleNeRF.volume_rendering (src/models/SimpleNeRF01.py:430-483) and
 * convert_depth_from_ndc (:486-502).
 *   sigma (n,S), rgb (n,S,3), depths (n,S)      device
 *   march_dirs (n,3)   rays_d, or rays_d_ndc when ndc      rays_o, rays_d (n,3) world rays, used only when ndc
 *   out_rgb (n,3), out_acc (n), out_depth (n), out_depth_var (n)             device, required
 *   out_depth_ndc (n), out_depth_var_ndc (n)                                  device, required when ndc
 *   out_alpha, out_visibility, out_weights (n,S)                              device, each may be NULL
 */
int snerf_composite(const float* sigma, const float* rgb, const float* depths, const float* march_dirs,
                    const float* rays_o, const float* rays_d, long long num_rays, int num_samples, int ndc,
                    int white_bkgd, float* out_rgb, float* out_acc, float* out_alpha, float* out_visibility,
                    float* out_weights, float* out_depth, float* out_depth_var, float* out_depth_ndc,
                    float* out_depth_var_ndc, snerf_stream_t stream);

/* K6  backward of the compositing (autograd of volume_rendering :446-460): per-ray gradients of rgb / acc / depth /
 * depth_ndc (each (n,3) or (n), any may be NULL = zero) -> d_sigma (n,S), d_rgb (n,S,3).  `depth` is the world depth
 * for NDC scenes, as in the forward.  No gradient is produced for depth_var* (no reference loss reads them).
 */
int snerf_composite_backward(const float* sigma, const float* rgb, const float* depths, const float* march_dirs,
                             const float* rays_o, const float* rays_d, long long num_rays, int num_samples, int ndc,
                             int white_bkgd, const float* grad_rgb, const float* grad_acc, const float* grad_depth,
                             const float* grad_depth_ndc, float* d_sigma, float* d_rgb, snerf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K5  hierarchical resampling.  Replaces SimpleNeRF.get_z_vals_fine (src/models/SimpleNeRF01.py:304-315) and
 * sample_pdf (:329-361): inverse-CDF samples of the coarse weights merged with the coarse depths, ascending.
 *   depths_coarse, weights_coarse  device (n, num_coarse)
 *   u            device (n, num_fine) uniform draws (:341), or NULL for the deterministic linspace of :338
 *   depths_fine  device (n, num_coarse + num_fine)
 */
int snerf_resample_depths(const float* depths_coarse, const float* weights_coarse, long long num_rays,
                          int num_coarse, int num_fine, const float* u, float* depths_fine, snerf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The one-call render ops (SURVEY 8b "Ownership / errors": render_forward / render_backward).
 *
 * snerf_render_forward enqueues on ONE stream everything SimpleNeRF.render_rays does for a batch of rays
 * (src/models/SimpleNeRF01.py:108-270): coarse depths (K2) -> for the main coarse MLP and, when present, the points- and
 * views-augmentation coarse MLPs: fused encoding + MLP (K3) and compositing (K4) -> inverse-CDF resampling of the main
 * coarse weights + merge (K5) -> the same for the fine-level MLPs on the merged depths.  snerf_render_backward enqueues
 * what autograd replays for it: per level the compositing backward (K6) and the MLP parameter-gradient backward (K7).
 * Like every entry point they only enqueue: no allocation, no synchronisation; every buffer is the caller's.
 *
 * Levels (the six MLPs a SimpleNeRF model can hold, :17-41): a NULL `desc` means the level is absent.  Levels 1, 2, 4, 5
 * are the augmentation models, which the reference evaluates in training mode only -- the caller passes them only then.
 */
enum snerf_render_level {
    SNERF_LEVEL_MAIN_COARSE = 0, SNERF_LEVEL_POINTS_AUG_COARSE = 1, SNERF_LEVEL_VIEWS_AUG_COARSE = 2,
    SNERF_LEVEL_MAIN_FINE = 3, SNERF_LEVEL_POINTS_AUG_FINE = 4, SNERF_LEVEL_VIEWS_AUG_FINE = 5
};
#define SNERF_RENDER_LEVELS 6

typedef struct snerf_render_config {
    int ndc;              /* configs['data_loader']['ndc'] */
    int white_bkgd;       /* model.white_bkgd (:462-463) */
    int lindisp;          /* model.lindisp (:286-289) */
    int num_coarse;       /* coarse_mlp.num_samples */
    int num_fine;         /* fine_mlp.num_samples, or 0 when the model has no fine MLP */
    int precision;        /* enum snerf_precision, for every MLP of the call */
    int keep_activations; /* != 0: training forward (snerf_mlp_forward_train); level outputs need `saved_acts` */
    int fused;            /* != 0: an eval-mode render of a plain coarse + fine model (levels 0 and 3 only, 64+128 or 128+128
                             samples, no noise / visibility / fine-depth override; SNERF_PRECISION_FP32 with the view-dependent
                             8 x 256 / 4 x 128 layouts, or SNERF_PRECISION_F16 / F16S8 / BF16 / BF16S8 with the 8 x 256 one)
                             runs as ONE launch that keeps each ray group's sample tile in LDS from the coarse depths to the
                             fine colour (csrc/render_fused.hip);
                             bit-identical outputs; `sigma` / `raw_rgb` of the two levels may then be NULL (not produced).
                             Any other call takes the stage-by-stage path as if the flag were 0 */
} snerf_render_config;

typedef struct snerf_render_mlp {
    const snerf_mlp_desc* desc; /* NULL = level absent */
    const float* packed;        /* device, snerf_mlp_pack's stream for that descriptor */
} snerf_render_mlp;

typedef struct snerf_render_rays {          /* device pointers, layouts of the reference's input_batch (:113-137) */
    const float *rays_o, *rays_d;           /* (n,3) world rays */
    const float* view_dirs;                 /* (n,3), or NULL when no MLP uses view directions */
    const float *rays_o_ndc, *rays_d_ndc;   /* (n,3), required when ndc */
    const float *near, *far;                /* (n): the columns the depths are spaced between (near_ndc/far_ndc when ndc) */
    const float* t_rand;                    /* (n, num_coarse) stratified-jitter draws (:299) or NULL */
    const float* u;                         /* (n, num_fine) inverse-CDF draws (:341) or NULL (deterministic linspace) */
    const float* sigma_noise[SNERF_RENDER_LEVELS]; /* per level (n, S) density noise, already scaled (:669-672), or NULL */
    const float* depths_fine;               /* (n, num_coarse+num_fine): use these fine depths instead of resampling
                                               (parity-test hook: sample_pdf has a rounding-dependent discontinuity), or NULL */
    const float* rays_o2;                   /* (n, num_other, 3) secondary camera centres ('rays_o2', :120-133) for the
                                               predict_visibility MLPs when sec_views_vis, or NULL */
    int num_other;                          /* num_frames - 1; 0 = no secondary views */
} snerf_render_rays;

typedef struct snerf_render_level_out {     /* S = num_coarse for levels 0-2, num_coarse + num_fine for levels 3-5 */
    float *rgb, *acc, *depth, *depth_var;   /* (n,3), (n), (n), (n): required for a present level */
    float *depth_ndc, *depth_var_ndc;       /* (n): required when ndc */
    float *alpha, *visibility, *weights;    /* (n,S): each may be NULL */
    float *sigma, *raw_rgb;                 /* (n,S), (n,S,3): the MLP outputs ('raw_sigma', 'raw_rgb'), required */
    float* saved_acts;                      /* snerf_mlp_saved_floats(desc, n, S) floats, required when keep_activations */
    float* raw_visibility;                  /* (n,S): predict_visibility levels, may be NULL */
    float* raw_visibility2;                 /* (n,S,num_other): required for such a level when rays.num_other > 0 */
    float* visibility2;                     /* (n,num_other): composited, required with raw_visibility2 */
    float* view_dirs2;                      /* (n,S,num_other,3) scratch, required with raw_visibility2 */
} snerf_render_level_out;

typedef struct snerf_render_outputs {
    float* depths_coarse;                   /* (n, num_coarse) 'z_vals_coarse', required */
    float* depths_fine;                     /* (n, num_coarse+num_fine) 'z_vals_fine'; required when num_fine > 0 and
                                               rays.depths_fine is NULL */
    snerf_render_level_out level[SNERF_RENDER_LEVELS];
} snerf_render_outputs;

/* Scratch of snerf_render_forward in floats (the main coarse weights, when level[0].weights is NULL).
 *
 * Round 5: below 65 536 coarse samples per call (num_rays x num_coarse) and with more than two MLP levels, snerf_render_forward and
 * snerf_render_backward run the levels SIDE BY SIDE on streams of the library's own -- forward {main coarse -> fine} | points-aug
 * | views-aug, backward every level -- forked from `stream` and joined back to it with events before the call returns: the call
 * is still enqueue-only, work enqueued on `stream` afterwards is ordered after all of it, and a graph capture of `stream`
 * records the side streams as parallel branches.  Results are bit-identical to the levels in order.  The side streams and
 * events are created on first use per (device, stream) and kept for the life of the process (at most 64 sets; further caller
 * streams get the levels in order). */
size_t snerf_render_workspace_floats(const snerf_render_config* cfg, long long num_rays);
int snerf_render_forward(const snerf_render_config* cfg, const snerf_render_mlp* mlps, const snerf_render_rays* rays,
                         long long num_rays, const snerf_render_outputs* out, float* workspace, snerf_stream_t stream);

typedef struct snerf_render_level_grads {   /* dL/d(output) of one level, each (shape as the output) or NULL = zero */
    const float *rgb, *acc, *depth, *depth_ndc, *sigma, *raw_rgb;
    float* const* param_grads;              /* the level's parameter gradients, as snerf_mlp_backward; NULL = skip level */
    int num_params;
    int accumulate;                         /* as snerf_mlp_backward */
} snerf_render_level_grads;

/* Scratch of snerf_render_backward in floats: d sigma + d rgb of the largest level + the largest snerf_mlp_backward
 * workspace among the present levels (levels run one after another on the stream and share it); for a call whose levels run
 * side by side (above) the SUM over the levels -- each level its own region.  Always ask this function. */
size_t snerf_render_backward_workspace_floats(const snerf_render_config* cfg, const snerf_render_mlp* mlps, long long num_rays);
/* `out` = the buffers snerf_render_forward (keep_activations != 0) filled for the same cfg / mlps / rays.  A level whose
 * param_grads is NULL, or whose six gradient pointers are all NULL, is skipped (its param_grads are not touched). */
int snerf_render_backward(const snerf_render_config* cfg, const snerf_render_mlp* mlps, const snerf_render_rays* rays,
                          long long num_rays, const snerf_render_outputs* out, const snerf_render_level_grads* grads,
                          float* workspace, snerf_stream_t stream);

/* The output layout of a render call (added within ABI version 10): which outputs exist, their shapes, and where each one
 * lies in the two pools a caller allocates -- every per-ray output of every level in one buffer, every per-sample output in
 * another.  Host arithmetic only (csrc/render_layout.h); no device is touched.  Every pooled output is (n, dims...) row-major and
 * all sizes are in floats PER RAY, so a layout holds for any ray count: an output begins n * unit_offset floats into its pool,
 * and a pool holds n * pool_unit_floats floats. */
enum snerf_render_field {                   /* the fields of snerf_render_level_out, in declaration order */
    SNERF_FIELD_RGB = 0, SNERF_FIELD_ACC, SNERF_FIELD_DEPTH, SNERF_FIELD_DEPTH_VAR, SNERF_FIELD_DEPTH_NDC,
    SNERF_FIELD_DEPTH_VAR_NDC, SNERF_FIELD_ALPHA, SNERF_FIELD_VISIBILITY, SNERF_FIELD_WEIGHTS, SNERF_FIELD_SIGMA,
    SNERF_FIELD_RAW_RGB, SNERF_FIELD_SAVED_ACTS, SNERF_FIELD_RAW_VISIBILITY, SNERF_FIELD_RAW_VISIBILITY2,
    SNERF_FIELD_VISIBILITY2, SNERF_FIELD_VIEW_DIRS2
};
#define SNERF_RENDER_FIELDS 16
enum snerf_render_pool { SNERF_POOL_PER_RAY = 0, SNERF_POOL_PER_SAMPLE = 1, SNERF_POOL_OWN = 2 };

typedef struct snerf_render_slot {
    long long unit_offset;                  /* floats per ray from the start of its pool (0 for SNERF_POOL_OWN) */
    int present;                            /* != 0: the call produces (or needs room for) this output */
    int returned;                           /* != 0: the caller sees it; 0: scratch (view_dirs2, the weights carved only because
                                               visibility2 is composited with them) and saved_acts */
    int pool;                               /* enum snerf_render_pool; SNERF_POOL_OWN (saved_acts): an allocation of its own of
                                               snerf_mlp_saved_floats floats, not linear in n */
    int rank;                               /* trailing dimensions after n: 0..3 */
    int dims[3];
} snerf_render_slot;

typedef struct snerf_render_layout {
    int num_fine;                           /* cfg.num_fine, or 0 when the main fine level is absent */
    int samples[SNERF_RENDER_LEVELS];       /* S of each level */
    int needs_workspace;                    /* != 0: snerf_render_forward needs snerf_render_workspace_floats of scratch */
    long long pool_unit_floats[2];          /* per-ray pool, per-sample pool */
    snerf_render_slot depths_coarse, depths_fine;   /* depths_fine is absent without a fine pass or when the caller supplies it */
    snerf_render_slot level[SNERF_RENDER_LEVELS][SNERF_RENDER_FIELDS];
} snerf_render_layout;

/* Of `mlps` only desc != NULL and desc->predict_visibility are read.  per_sample_mask: 1 alpha | 2 visibility | 4 weights.
 * fine_depths_given != 0: the call passes rays.depths_fine. */
int snerf_render_layout_query(const snerf_render_config* cfg, const snerf_render_mlp* mlps, int num_other, int per_sample_mask,
                              int fine_depths_given, snerf_render_layout* layout);
/* Points every pooled output of `out` into the two pools; absent outputs and saved_acts become NULL. */
int snerf_render_layout_bind(const snerf_render_layout* layout, long long num_rays, float* per_ray_pool, float* per_sample_pool,
                             snerf_render_outputs* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Output post-processing (next-row f3).  Replaces post_process_image / post_process_depth
 * (src/data_preprocessors/DataPreprocessor01.py:1106-1114) on the device, so a rendered frame crosses PCIe as uint8.
 *   rgb (n,3) device; depth (n) device or NULL;  image (n,3) uint8 device;  depth_out (n) device or NULL
 *   image (and rgb) may be NULL to convert a depth column alone (retrieve_inference_outputs :906-918 converts four).
 * Pinned edge cases (tests/golden/display.npz, made by the reference's functions): colour NaN -> 0, +inf -> 255,
 * exact .5 ties round to even; depth NaN stays NaN, -0.0 stays -0.0, -inf -> 0.
 */
int snerf_to_display(const float* rgb, const float* depth, long long num_rays, unsigned char* image, float* depth_out,
                     snerf_stream_t stream);

/* The trainer's 8-bit previews (rint(x / max(x) * 255) over whole maps; snerf_maps_to_u8) are an entry point of the same library
 * that is NOT declared in this header: the set of prototypes here is pinned, so it has a header of its own,
 * simplenerf_amd/csrc/simplenerf_maps.h, which the Python binding reads after this one. */

/* ---------------------------------------------------------------------------------------------------------------
 * Q1  scoring a rendered frame on the device: the sums behind the reference's frame metrics (src/qa/01_RMSE, 02_PSNR,
 * 03_SSIM, 05_DepthRMSE, 06_DepthMAE, 07_DepthSROCC and their masked forms 11-13, 15-17); the host turns them into the
 * metrics (simplenerf_amd/qa.py).  These functions were ADDED within ABI version 10: no existing struct or signature
 * changed, so SNERF_ABI_VERSION stays 10 (a caller that needs them checks that the symbol exists).
 *   gt, eval   device (height, width, 3) uint8 -- the image layout of the display conversion above -- or device (count) fp32 depths
 *   mask       device (height, width) / (count) bytes, non-zero = counted; NULL = no mask
 *   workspace  device scratch, at least the workspace-bytes query below for the frame (for the 1-D calls: any height * width >=
 *              count); no initial state is needed, and calls enqueued on ONE stream may share it
 * Image sums are exact 64-bit integers, everything else is fp64; every reduction folds per-workgroup partial sums in a
 * fixed order (no atomics), so two calls on the same input return the same bits.  Like every entry point these only
 * enqueue on `stream`: no allocation, no synchronisation; a non-zero return leaves its message for the last-error query.
 */
long long snerf_metrics_workspace_bytes(int height, int width);

/* sums  device (3) int64: sum (gt - eval)^2 over all height*width*3 values; the same over the masked pixels; number of masked
 *       pixels (both 0 without a mask).  MSE = sums[0] / (3 height width), masked MSE = sums[1] / (3 sums[2]). */
int snerf_image_error_sums(const unsigned char* gt, const unsigned char* eval, const unsigned char* mask, int height,
                           int width, long long* sums, void* workspace, snerf_stream_t stream);

/* Gaussian-weighted SSIM map S per channel as skimage's structural_similarity computes it with gaussian_weights=True,
 * sigma=1.5, use_sample_covariance=False, data_range=255: an 11-tap separable window (truncate 3.5) with scipy's `reflect`
 * boundary, v = E[x^2] - E[x]^2, S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)).  With a mask, eval is
 * replaced by gt on the unmasked pixels first (13_MaskedSSIM).  height, width >= 11.
 *   sums   device (2) fp64: sum of S over the map cropped by 5 pixels on every side (SSIM = sums[0] / (3 (height-10)(width-10)));
 *          sum of S over the masked pixels of the whole map (MaskedSSIM = sums[1] / (3 #masked)) -- over every pixel without a mask
 *   s_map  device (height, width, 3) fp64 or NULL: the whole map S, border included */
int snerf_ssim_sums(const unsigned char* gt, const unsigned char* eval, const unsigned char* mask, int height, int width,
                    double* sums, double* s_map, void* workspace, snerf_stream_t stream);

/* e = gt * gt_scale - eval * eval_scale in fp64 (the per-side factors of the reference's get_depth_scale, applied first).
 *   sorted_gt  device (count): gt sorted ascending, or NULL when the median is not wanted
 *   sums       device (4) fp64: sum |e|, sum e^2, number of pixels counted (masked, or all); numpy.median(gt * gt_scale) over ALL of
 *              gt, mask or not (mean of the two middle values for an even count; untouched when sorted_gt is NULL) */
int snerf_depth_error_sums(const float* gt, const float* eval, double gt_scale, double eval_scale, const unsigned char* mask,
                           long long count, const float* sorted_gt, double* sums, void* workspace, snerf_stream_t stream);

/* Spearman's rank correlation of (x, y) from tie-averaged ranks: the rank of each value is found in the sorted copy by a lower
 * and an upper bound search (no walk along a run of ties) and centred by the exact mean rank (count + 1) / 2.
 *   sorted_x, sorted_y  device (count): x and y sorted ascending
 *   sums  device (3) fp64: sum rx ry, sum rx^2, sum ry^2;  SROCC = sums[0] / sqrt(sums[1] sums[2]) */
int snerf_rank_correlation_sums(const float* x, const float* y, const float* sorted_x, const float* sorted_y, long long count,
                                double* sums, void* workspace, snerf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Q2  the visibility mask of the masked metrics: the reference's src/qa/00_Common/src/mask_generators (Warper.forward_warp,
 * MaskComputer.compute_mask, "visible in at least two training views").  `views` training depths are splatted into ONE test view of
 * the same resolution and tested against its depth.  Like Q1 these were ADDED within ABI version 10 (no existing struct or
 * signature changed; a caller checks that the symbol exists).  The call sequence is project -> a STABLE ascending sort of `keys`
 * by the caller (sorted keys + the permutation, e.g. torch.sort(keys, stable=True)) -> list_starts -> gather -> combine, all on one
 * stream.  All arithmetic is fp64 (fp32 depths are widened on load); there is no floating-point atomic: every destination pixel
 * sums its sources in ascending source order, so two calls on the same input return the same bits.  The calls only enqueue on
 * `stream`: no allocation, no synchronisation.  views * ((height + 1)(width + 1) + 1) must stay below 2^31, views <= 65535.
 *
 * Conventions.  Extrinsics are 4x4 world-to-camera [R t; 0 1], intrinsics 3x3 [f 0 cx; 0 f cy; 0 0 1], x right, y down, z forward,
 * as in the database's CameraExtrinsics.csv / CameraIntrinsics.csv; depths are z-depths in the extrinsics' units.  The HOST inverts
 * and composes them in fp64:
 *   cameras  device (views, 30) fp64, row-major per view: inv(K_train) 3x3 | rows 0..2 of E_test inv(E_train) 3x4 | K_test 3x3
 * Source pixel (x, y) of a view: p = inv(K_train) (x, y, 1)^T d_train[y, x], q = K_test (T (p, 1))[:3]; padded position
 * (X, Y) = (q0 / q2 + 1, q1 / q2 + 1), transformed depth Z = q2.  It adds prox / exp(50 L / max L), L = log(1 + clip(Z, 0, 1000)),
 * max over the view's sources, to the cells (floor | ceil X, floor | ceil Y) clipped to the padded (height + 2, width + 2) grid
 * (floor and ceil before the clip; an integer coordinate adds twice to one cell), prox = the bilinear proximity of the clipped
 * position; the padded border is cropped.  Kept as the reference has it: a point behind the test camera (Z < 0) still splats,
 * with the LARGEST depth weight (its L is 0).  Not pinned by the reference (undefined there): a source whose X, Y or Z is not
 * finite or whose floor leaves int32, and a view whose max L is 0 -- such a source, or every source of such a view, adds nothing.
 */
long long snerf_visibility_mask_workspace_bytes(int views, int height, int width);

/* depth_train  device (views, height, width) fp32
 * points       device (views, 3, height, width) fp64, written: the planes X, Y, Z of every source
 * keys         device (views, height, width) int32, written: view * ((height+1)(width+1) + 1) + the source's list -- its unclipped
 *              floor cell fy * (width + 1) + fx when that lies in [0, height] x [0, width] (only those can reach a cell that survives
 *              the crop), else (and for an unpinned source) the view's last key, the discard list that is never walked
 * stats        device (views, 2) fp64, written: max L, max d_train (of the untransformed depth) per view
 * workspace    device scratch of at least the query above; no initial state */
int snerf_visibility_mask_project(const float* depth_train, const double* cameras, int views, int height, int width, double* points,
                                  int* keys, double* stats, void* workspace, snerf_stream_t stream);

/* sorted_keys  device (views * height * width) int32: `keys` sorted ascending
 * starts       device (views * ((height+1)(width+1) + 1) + 1) int32, written: starts[k] = first sorted position whose key is >= k */
int snerf_visibility_mask_list_starts(const int* sorted_keys, int views, int height, int width, int* starts, snerf_stream_t stream);

/* order         device (views * height * width) int64: the permutation of the STABLE sort (sorted position -> index into `keys`)
 * depth_test    device (height, width) fp32
 * mask_views    device (views, height, width) bytes, written: 1 where weight_sum > 0 and
 *               |warped_depth - depth_test| < depth_error_threshold * max d_train of that view
 * warped_depth  device (views, height, width) fp64 or NULL: sum Z weight / sum weight where weight_sum > 0, else 0
 * weight_sum    device (views, height, width) fp64 or NULL: sum of the weights that landed on the pixel */
int snerf_visibility_mask_gather(const double* points, const long long* order, const int* starts, const double* stats,
                                 const float* depth_test, double depth_error_threshold, int views, int height, int width,
                                 unsigned char* mask_views, double* warped_depth, double* weight_sum, snerf_stream_t stream);

/* mask  device (height, width) bytes, written: 1 where at least min_views (1 .. views) of mask_views are set; the reference's
 *       numpy.sum(masks, axis=0) > 1 is min_views = 2 */
int snerf_visibility_mask_combine(const unsigned char* mask_views, int views, int height, int width, int min_views,
                                  unsigned char* mask, snerf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Q3  LPIPS of a rendered frame on the device: lpips.LPIPS(net='alex'), version 0.1, lin layers on, eval mode, spatial=False, as
 * the reference's src/qa/04_LPIPS and 14_MaskedLPIPS call it on the 8-bit frames.  Like Q1 and Q2 these were ADDED within ABI
 * version 10 (no existing struct or signature changed; a caller checks that the symbol exists).  The library carries no weights:
 * the caller passes torchvision's AlexNet convolutions and the package's lin layers, and snerf_lpips_pack re-orders them once.
 *
 *   x = u * 2 / 255 - 1 (fp32, in that order), (x - shift) / scale per channel; conv 3->64 k11 s4 p2 | pool, conv 64->192 k5 p2 |
 *   pool, conv 192->384 k3 p1 | conv 384->256 k3 p1 | conv 256->256 k3 p1, every conv with bias and ReLU, pool = 3 x 3 stride 2
 *   maximum without padding (floor mode); per layer l and pixel v = sum_c lin_l[c] (f_gt[c] / (|f_gt| + 1e-10) - f_eval[c] /
 *   (|f_eval| + 1e-10))^2 over the post-ReLU features; LPIPS = sum_l mean over the layer's pixels of v.
 *
 * The convolutions run on the fp32 matrix cores as implicit GEMMs over NHWC activations; every sum (the k sum of an output
 * element, the channel sums, the pixel sums) runs in one fixed order without atomics, so two calls on the same input return the
 * same bits, and exchanging gt and eval does too.  The calls only enqueue on `stream`: no allocation, no synchronisation.
 * height, width >= 31 (the smallest image the network accepts) and <= 16384.
 */
/* number of floats of the packed weight buffer */
long long snerf_lpips_packed_floats(void);

/* conv_weights  host array of 5 device pointers: (c_out, c_in, k, k) fp32, torch's layout (features.0/3/6/8/10.weight)
 * conv_biases   host array of 5 device pointers: (c_out) fp32
 * lin_weights   host array of 5 device pointers: (c_out) fp32 (lin{0..4}.model.1.weight, (1, c_out, 1, 1))
 * scaling       host array of 6 floats, shift[3] then scale[3], or NULL for the package's (-.030, -.088, -.188) / (.458, .448, .450)
 * packed        device, snerf_lpips_packed_floats() floats, written */
int snerf_lpips_pack(const float* const* conv_weights, const float* const* conv_biases, const float* const* lin_weights,
                     const float* scaling, float* packed, snerf_stream_t stream);

/* bytes of device scratch snerf_lpips_sums needs for a height x width frame (0 for an extent it refuses); no initial state */
long long snerf_lpips_workspace_bytes(int height, int width);

/* extents of layer's (0..4) post-ReLU tap for a height x width frame */
int snerf_lpips_tap_shape(int height, int width, int layer, int* tap_height, int* tap_width, int* channels);

/* gt, eval  device (height, width, 3) uint8;  mask  device (height, width) bytes or NULL: eval is replaced by gt where it is zero
 *           (14_MaskedLPIPS: an all-zero mask gives sums of exactly 0)
 * packed    what snerf_lpips_pack wrote
 * sums      device (5) fp64, written: per layer the sum of v over the tap's pixels; LPIPS = sum_l sums[l] / (tap_height_l tap_width_l)
 * taps      NULL, or a host array of 5 device pointers (each may be NULL): layer l's post-ReLU activations of both images are
 *           written there, fp32 (2, tap_height_l, tap_width_l, channels_l), gt first, channels last */
int snerf_lpips_sums(const unsigned char* gt, const unsigned char* eval, const unsigned char* mask, int height, int width,
                     const float* packed, double* sums, float* const* taps, void* workspace, snerf_stream_t stream);

/* The same five entry points with the backbone as an argument (ADDED within ABI version 10).  SNERF_LPIPS_ALEX behaves exactly as
 * the functions above do; SNERF_LPIPS_VGG16 is lpips.LPIPS(net='vgg'), version 0.1, lin layers on, eval mode, spatial=False:
 *
 *   the same scaling layer; torchvision's vgg16 `features`: thirteen 3 x 3 stride-1 pad-1 convolutions with bias and ReLU (indices
 *   0 2 | 5 7 | 10 12 14 | 17 19 21 | 24 26 28; channels 3->64 64->64 | 64->128 128->128 | 128->256 256->256 256->256 | 256->512
 *   512->512 512->512 | 512->512 512->512 512->512), a 2 x 2 stride-2 maximum (no padding, floor mode) at each `|`; the five taps
 *   are the ReLUs of convolutions 2, 7, 14, 21, 28 (64, 128, 256, 512, 512 channels); per tap and pixel the same v, LPIPS the
 *   same sum of means.
 *
 * height, width >= 16 (16 -> 8 -> 4 -> 2 -> 1) and <= 16384.  Any other selector is SNERF_E_INVALID (a count or a size of 0).
 * The arrays of snerf_lpips_net_pack hold 13 convolution weights ((c_out, c_in, 3, 3), in the order above) and biases and 5 lin
 * weights for VGG-16; `layer` of snerf_lpips_net_tap_shape and the entries of `taps` and `sums` count the five taps.  A packed
 * buffer belongs to the network it was packed for. */
enum { SNERF_LPIPS_ALEX = 0, SNERF_LPIPS_VGG16 = 1 };
long long snerf_lpips_net_packed_floats(int net);
int snerf_lpips_net_pack(int net, const float* const* conv_weights, const float* const* conv_biases, const float* const* lin_weights,
                         const float* scaling, float* packed, snerf_stream_t stream);
long long snerf_lpips_net_workspace_bytes(int net, int height, int width);
int snerf_lpips_net_tap_shape(int net, int height, int width, int layer, int* tap_height, int* tap_width, int* channels);
int snerf_lpips_net_sums(int net, const unsigned char* gt, const unsigned char* eval, const unsigned char* mask, int height, int width,
                         const float* packed, double* sums, float* const* taps, void* workspace, snerf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Q4  the sorts and the mask selection Q1 and Q2 consume: sorted depths for the median and the tie-averaged ranks
 * (snerf_depth_error_sums, snerf_rank_correlation_sums), the stable sort of the splat keys between snerf_visibility_mask_project and
 * _list_starts / _gather, and the selection of the masked pixels for the masked rank correlation.  Like Q1-Q3 these were ADDED
 * within ABI version 10 (no existing struct or signature changed; a caller checks that the symbol exists).
 *
 * The sort is a least-significant-digit radix sort on 8-bit digits, ceil(key_bits / 8) passes of count, scan, scatter.  It is
 * STABLE (equal keys keep their input order) and holds no atomic: the same input gives the same bits on every call.  The input is
 * never written; the passes alternate between the output and the workspace so that the last one lands in the output.  The calls
 * only enqueue on `stream`: no allocation, no synchronisation, no copy to the host.  count == 0 returns SNERF_OK at once (the
 * compaction still writes a kept count of 0); count < 0 or >= 2^31, key_bits outside 1..32 and a NULL pointer are
 * SNERF_E_INVALID before anything is enqueued.  Outputs must not overlap inputs.
 *   workspace  device scratch of at least the query below (256-byte aligned, as hipMalloc returns it); no initial state, and calls
 *              enqueued on ONE stream may share it
 */
/* bytes of scratch a sort of `count` keys of `key_bits` bits needs (key_bits = 32 for snerf_sort_f32); 0 for a count of 0 and for
 * what the sorts refuse.  Never decreases as count grows. */
long long snerf_sort_workspace_bytes(long long count, int key_bits);

/* sorted  device (count) fp32, written: `values` ascending by the total order -inf < ... < -0 < +0 < ... < +inf < NaN.  -0 comes
 *         before +0; every NaN, whatever its sign or payload, comes last and is returned as the quiet NaN 0x7FC00000.  On input
 *         without NaN and -0 this is torch.sort(values).values / numpy.sort(values), bit for bit. */
int snerf_sort_f32(const float* values, long long count, float* sorted, void* workspace, snerf_stream_t stream);

/* keys         device (count) int32, 0 <= key < 2^key_bits (bits from key_bits up, rounded up to a multiple of 8, are not looked at)
 * sorted_keys  device (count) int32, written: the keys ascending
 * order        device (count) int64, written: the permutation of the stable sort, sorted_keys[j] = keys[order[j]], ascending within a
 *              run of equal keys -- numpy.argsort(keys, kind='stable'); what snerf_visibility_mask_gather takes */
int snerf_sort_keys_with_order(const int* keys, long long count, int key_bits, int* sorted_keys, long long* order, void* workspace,
                               snerf_stream_t stream);

/* bytes of scratch snerf_compact_f32_pair needs for `count` positions (0 for a count of 0 and for what it refuses) */
long long snerf_compact_workspace_bytes(long long count);

/* a_kept[j] = a[i_j], b_kept[j] = b[i_j] for the ascending positions i_j whose mask byte is not zero (count, scan, scatter: the
 * output order is the input order).
 *   a, b            device (count) fp32;  mask  device (count) bytes
 *   a_kept, b_kept  device (count) fp32: the first kept[0] values are written, the rest is left alone
 *   kept            device (1) int64, written: the number of kept positions */
int snerf_compact_f32_pair(const float* a, const float* b, const unsigned char* mask, long long count, float* a_kept, float* b_kept,
                           long long* kept, void* workspace, snerf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Q5  the rest of the reference's Warper (src/qa/00_Common/src/mask_generators/Warper.py) on the device: forward_warp's colour frame
 * and flow, bilinear_splatting of any (height, width, channels) frame along any flow, and bilinear_interpolation, the backward warp.
 * Like Q1-Q4 these were ADDED within ABI version 10 (no existing struct or signature changed; a caller checks that the symbol
 * exists).  ONE frame per call; channels is 1..4; a frame is interleaved (height, width, channels); masks are bytes, non-zero = true,
 * and may be NULL (all true).  views = 1 in every Q2 / Q4 call of the recipes:
 *
 *   splat along a flow    snerf_warp_positions_from_flow -> snerf_sort_keys_with_order (or any STABLE sort of `keys`) ->
 *                         snerf_visibility_mask_list_starts(views = 1) -> snerf_warp_splat_gather
 *   forward_warp          snerf_warp_project -> the same sort and list starts, ONCE -> snerf_warp_splat_gather of the uint8 frame
 *                         (is_image) and snerf_warp_splat_gather of the Z plane of `points` (points + height * width, SNERF_WARP_F64,
 *                         1 channel): the warped depth, bit for bit what snerf_visibility_mask_gather returns for that view
 *   backward warp         snerf_warp_interpolate alone
 *
 * Semantics are Q2's (padded grid, floor and ceil before the clip, weight prox / exp(50 L / max L), a point behind the camera splats
 * with the largest weight).  A source whose mask1 or flow12_mask is false adds nothing (the reference multiplies its weight by 0),
 * yet max L is the maximum over ALL pixels of the depth, as the reference's log_depth1.max() is.  All arithmetic is fp64 on inputs
 * widened first and is compiled without FMA contraction: a position computed from a flow, (flow + grid) + 1, and every fp64 output
 * of snerf_warp_interpolate equal numpy's bit for bit; the splat differs from numpy by the rounding of exp / log and of the order
 * of its sums only.  No floating-point atomic: two calls on the same input return the same bits.  Not pinned by the reference
 * (undefined there) and given no contribution: a source or a backward-warped pixel whose position is not finite or leaves int32, a
 * source whose depth is not finite, a view whose max L is 0; with is_image a NaN value is stored as 0.  The calls only enqueue on
 * `stream`: no allocation, no synchronisation.  (height + 1)(width + 1) + 1 must stay below 2^31.
 */
enum { SNERF_WARP_U8 = 0, SNERF_WARP_F32 = 1, SNERF_WARP_F64 = 2 };

/* bytes of scratch snerf_warp_project / snerf_warp_positions_from_flow need (0 for an extent they refuse); no initial state */
long long snerf_warp_workspace_bytes(int height, int width);

/* The projection of snerf_visibility_mask_project for ONE view (the same kernel: points, keys and stats[0] are the bits that
 * call returns for the view when mask1 is NULL), which also writes the flow.
 *   depth1  device (height, width) fp32;  camera  device (30) fp64, one row of Q2's `cameras`;  mask1  device (height, width) or NULL
 *   points  device (3, height, width) fp64, written;  keys  device (height, width) int32, written (0 .. (height+1)(width+1), the last
 *           the discard list);  stats  device (2) fp64, written: max L, max depth1
 *   flow12  device (height, width, 2) fp64, written: (q0 / q2 - x, q1 / q2 - y) */
int snerf_warp_project(const float* depth1, const double* camera, const unsigned char* mask1, int height, int width, double* points,
                       int* keys, double* stats, double* flow12, void* workspace, snerf_stream_t stream);

/* X = (flow_x + x) + 1, Y = (flow_y + y) + 1, Z = depth1; outputs as above (stats[1] = max depth1).
 *   flow12  device (height, width, 2) fp64;  depth1  device (height, width) of depth_type SNERF_WARP_F32 or SNERF_WARP_F64
 *   mask1, flow12_mask  device (height, width) bytes or NULL */
int snerf_warp_positions_from_flow(const double* flow12, const void* depth1, int depth_type, const unsigned char* mask1,
                                   const unsigned char* flow12_mask, int height, int width, double* points, int* keys, double* stats,
                                   void* workspace, snerf_stream_t stream);

/* points, stats  as written above;  order  the int64 permutation of the STABLE sort of keys;  starts  snerf_visibility_mask_list_starts
 * values  device (height, width, channels) of value_type: what every source carries
 * warped  device (height, width, channels), written: sum v weight / sum weight where sum weight > 0, else 0 -- fp64, or with is_image
 *         (SNERF_WARP_U8 values only) clipped to [0, 255], rounded half to even, uint8
 * mask2   device (height, width) bytes, written: sum weight > 0 */
int snerf_warp_splat_gather(const double* points, const long long* order, const int* starts, const double* stats, const void* values,
                            int value_type, int channels, int is_image, int height, int width, void* warped, unsigned char* mask2,
                            snerf_stream_t stream);

/* Warper.bilinear_interpolation: warped[y, x] = nr / dr where dr > 0, else 0, over the four taps of the zero-padded frame2 / mask2 at
 * the padded position ((flow_x + x) + 1, (flow_y + y) + 1), nr = sum prox flow12_mask frame2 mask2, dr = sum prox flow12_mask mask2,
 * both added in the order nw, sw, ne, se.  warped as above (fp64, or uint8 with is_image); mask1 bytes, written: dr > 0. */
int snerf_warp_interpolate(const void* frame2, int value_type, int channels, const unsigned char* mask2, const double* flow12,
                           const unsigned char* flow12_mask, int is_image, int height, int width, void* warped, unsigned char* mask1,
                           snerf_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Opt-in event timing of the dominant kernels (the measurement row, SURVEY 8d: "achieved" of the roofline is measured
 * live with HIP events on the stream the kernel is launched on).  While enabled, every snerf_mlp_forward[_train] launch
 * (kind SNERF_PROFILE_MLP_FORWARD) and every snerf_mlp_backward call (SNERF_PROFILE_MLP_BACKWARD) -- also those issued
 * from inside snerf_render_forward / _backward -- is bracketed by an event pair owned by the library.
 *   snerf_profile_enable(capacity)   create `capacity` event pairs and start recording; capacity <= 0 stops and frees
 *   snerf_profile_collect(kind, ms, samples, capacity)   waits for the recorded events of that kind and writes each
 *        launch's duration in milliseconds and its number of samples (rays x samples); returns how many, or < 0
 *   snerf_profile_reset()            forget the recorded launches (and the dropped count), keep recording
 *   snerf_profile_dropped()          launches since enable / reset that were NOT timed because all `capacity` pairs were in
 *                                    use -- a measurement whose count is not zero under-counts kernel time and FLOPs
 * Process-wide, off by default (one relaxed atomic load on the launch path).  Launches enqueued on a stream that is being
 * captured into a graph are never timed (hipStreamIsCapturing), so the hooks may stay enabled across a capture. */
enum snerf_profile_kind { SNERF_PROFILE_MLP_FORWARD = 0, SNERF_PROFILE_MLP_BACKWARD = 1 };
int snerf_profile_enable(int capacity);
int snerf_profile_collect(int kind, float* milliseconds, long long* samples, int capacity);
int snerf_profile_reset(void);
long long snerf_profile_dropped(void);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLENERF_HIP_H */
