// snerf_view_sweep (simplenerf_sweep.h): one pose under the view directions of V cameras, from the `feature` tiles a storing fp32
// forward has left in the saved activations.  Four launches, all in stream order:
//   1. sweep_transpose_kernel   W_v[:, :W] -> k-major wvt[i][j] in the workspace (the A operand rows of the matrix-core loop)
//   2. sweep_view_bias_kernel   (view_sweep_tail.h) u[v,n,:] = b_v + W_v[:, W:] . PE(d[v,n]), one wave per (view, ray)
//   3. sweep_block_kernel       one wave per 32-sample block: g = W_v[:, :W] . feature on v_mfma_f32_32x32x2_f32 -- the saved
//                               [feature][32 samples] tile IS the B operand -- kept in VT accumulator tiles while the loop over the
//                               views adds u, applies the ReLU and the 3 x Wv head on the VALU and writes weights * rgb per sample
//                               (sweep_tail, view_sweep_tail.h: shared with the 16-bit sweep)
//   4. sweep_fold_kernel        (view_sweep_tail.h) out[v,n,c] = the samples' products summed s = 0 .. S-1 by one thread: a fixed
//                               order that does not depend on how the ray's samples fall into the 32-sample blocks
// DESIGN.md section 9 has the reasons for each choice and the measured numbers.
#include "mlp_device.h"
#include "simplenerf_sweep.h"
#include "view_sweep_tail.h"
#include "wave.h"

namespace {

struct SweepArgs {
    const float* acts;        // saved activations, [block][act_rows][32]
    const float* weights;     // (total)
    const float* wvt;         // workspace: [W][Wv]
    const float* u;           // workspace: [V][n][Wv]
    const float* wo;          // views_output_linear.weight (3, Wv)
    const float* bo;          // views_output_linear.bias (3)
    float* products;          // workspace: [V][3][total]
    long long total, blocks, num_rays;
    int samples, views, act_rows, act_feature;
};

__global__ void __launch_bounds__(256) sweep_transpose_kernel(const float* __restrict__ wv, int ld, int width, int views_width,
                                                              float* __restrict__ wvt) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= width * views_width) return;
    const int i = t / views_width, j = t - i * views_width;
    wvt[t] = wv[(long long)j * ld + i];
}

// Four waves per workgroup, one 32-sample block each (neighbouring blocks: the four waves read the same rows of wvt at about the
// same time).  Lane (j = lane & 31, h = lane >> 5) holds sample j; accumulator register r of tile t is output feature
// 32 t + (r & 3) + 8 (r >> 2) + 4 h (mlp_layout.h), so a lane half owns every other group of four features.
// At least two waves per SIMD (launch bounds): a single wave has nobody to hide the loads of the matrix-core loop behind.
template <int WT, int VT>
__global__ void __launch_bounds__(256, 2) sweep_block_kernel(SweepArgs a) {
    constexpr int W = 32 * WT, WV = 32 * VT;
    __shared__ __attribute__((aligned(16))) float head[3 * WV + 4];
    for (int i = threadIdx.x; i < 3 * WV + 3; i += 256) head[i] = i < 3 * WV ? a.wo[i] : a.bo[i - 3 * WV];
    __syncthreads();
    const long long block = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (block >= a.blocks) return;          // (whole waves)
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;

    // g: 32 samples x Wv, K = W in W / 2 steps of two features (2 ks + h)
    const float* feat = a.acts + (block * a.act_rows + a.act_feature) * 32 + h * 32 + j;
    const float* wrow = a.wvt + h * WV + j;
    f32x16 acc[VT];
#pragma unroll
    for (int t = 0; t < VT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
#pragma unroll 4
    for (int ks = 0; ks < W / 2; ++ks) {
        const float b = feat[ks * 64];
#pragma unroll
        for (int t = 0; t < VT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[ks * 2 * WV + 32 * t], b, acc[t], 0, 0, 0);
    }

    // the lane's sample: a block may hold samples of several rays, and the last block of a call is partial
    const long long sample = block * 32 + j;
    const bool live = sample < a.total;
    const long long ray = live ? sample / a.samples : a.num_rays - 1;
    const float weight = live ? a.weights[sample] : 0.0f;
    sweep_tail<VT>(acc, head, a.u, a.products, sample, live, ray, weight, a.num_rays, a.total, a.views, h);
}

struct SweepPlan {
    snerf::MlpPlan mlp;
    long long wvt_floats = 0, u_floats = 0, product_floats = 0;
    long long total() const { return wvt_floats + u_floats + product_floats; }
};

int plan_sweep(const snerf_mlp_desc* desc, long long num_rays, int num_samples, int num_views, SweepPlan* out) {
    if (!desc) return snerf::fail(SNERF_E_INVALID, "view_sweep: NULL descriptor");
    SweepPlan p;
    const int st = snerf::build_plan(desc, &p.mlp);
    if (st == SNERF_E_UNSUPPORTED)
        return snerf::fail(SNERF_E_UNSUPPORTED, "view_sweep: built for the fused fp32 layouts only (points_net_width / views_net_width 256 / 128 "
                           "or 128 / 64, views_net_depth 1), not for a layered shape (width %d, views depth %d, views width %d)",
                           desc->points_net_width, desc->views_net_depth, desc->views_net_width);
    if (st != SNERF_OK) return st;
    const snerf::MlpPlan& m = p.mlp;
    if (!m.view_dependent)
        return snerf::fail(SNERF_E_UNSUPPORTED, "view_sweep: the MLP has no views head (view_dependent_rgb = 0): its colour does not "
                           "depend on the view direction");
    if (m.sigma_pe)
        return snerf::fail(SNERF_E_UNSUPPORTED, "view_sweep: sigma_pe_degree %d not built (-1): the views layer of a points-augmentation "
                           "layout also reads the point encoding", desc->sigma_pe_degree);
    if (desc->predict_visibility)
        return snerf::fail(SNERF_E_UNSUPPORTED, "view_sweep: predict_visibility MLPs are not built");
    if (!((m.width == 256 && m.views_width == 128) || (m.width == 128 && m.views_width == 64)))
        return snerf::fail(SNERF_E_UNSUPPORTED, "view_sweep: points_net_width / views_net_width %d / %d not built (256 / 128 or 128 / 64)",
                           m.width, m.views_width);
    SNERF_REQUIRE(num_rays >= 0, "view_sweep: num_rays %lld < 0", num_rays);
    SNERF_REQUIRE(num_samples >= 1, "view_sweep: num_samples %d < 1", num_samples);
    SNERF_REQUIRE(num_views >= 0, "view_sweep: num_views %d < 0", num_views);
    SNERF_REQUIRE(num_rays <= (1ll << 40) / num_samples, "view_sweep: %lld rays x %d samples: too many samples for one call", num_rays,
                  num_samples);
    p.wvt_floats = (long long)m.width * m.views_width;
    p.u_floats = round64((long long)num_views * num_rays * m.views_width);
    p.product_floats = round64((long long)num_views * 3 * num_rays * num_samples);
    *out = p;
    return SNERF_OK;
}

}  // namespace

extern "C" size_t snerf_view_sweep_workspace_floats(const snerf_mlp_desc* desc, long long num_rays, int num_samples, int num_views) {
    SweepPlan p;
    if (plan_sweep(desc, num_rays, num_samples, num_views, &p) != SNERF_OK) return 0;
    return (size_t)p.total();
}

extern "C" int snerf_view_sweep(const snerf_mlp_desc* desc, const float* const* params, int num_params, const float* saved_acts,
                                const float* weights, const float* acc, const float* view_dirs, long long num_rays,
                                int num_samples, int num_views, int white_bkgd, float* out_rgb, float* workspace,
                                snerf_stream_t stream) {
    SweepPlan p;
    const int st = plan_sweep(desc, num_rays, num_samples, num_views, &p);
    if (st != SNERF_OK) return st;
    const snerf::MlpPlan& m = p.mlp;
    if (num_rays == 0 || num_views == 0) return SNERF_OK;
    SNERF_REQUIRE(params, "view_sweep: NULL params");
    SNERF_REQUIRE(num_params == m.num_params, "view_sweep: %d parameter tensors, the descriptor has %d", num_params, m.num_params);
    const int pv = 2 * m.depth + 4;       // views_linears.0.weight, .bias, views_output_linear.weight, .bias
    for (int i = pv; i < pv + 4; ++i) SNERF_REQUIRE(params[i], "view_sweep: params[%d] is NULL", i);
    SNERF_REQUIRE(!white_bkgd || acc, "view_sweep: white_bkgd needs acc (NULL)");
    SNERF_REQUIRE(saved_acts && weights && view_dirs && out_rgb && workspace, "view_sweep: NULL pointer (saved_acts, weights, view_dirs, "
                  "out_rgb or workspace)");
    SNERF_REQUIRE(((unsigned long long)workspace & 15) == 0, "view_sweep: workspace must be 16-byte aligned");
    const long long total = num_rays * num_samples, pairs = (long long)num_views * num_rays;
    SNERF_REQUIRE(pairs * 3 < (1ll << 40), "view_sweep: %d views x %lld rays: too many for one call", num_views, num_rays);
    hipStream_t s = (hipStream_t)stream;
    const int ld = m.width + m.views_pe;
    float* wvt = workspace;
    float* u = wvt + p.wvt_floats;
    float* products = u + p.u_floats;

    hipLaunchKernelGGL(sweep_transpose_kernel, dim3((unsigned)((p.wvt_floats + 255) / 256)), dim3(256), 0, s, params[pv], ld, m.width,
                       m.views_width, wvt);
    hipLaunchKernelGGL(sweep_view_bias_kernel<kSweepFp32>, dim3((unsigned)(pairs < 65536 ? pairs : 65536)), dim3(64), 0, s, params[pv],
                       params[pv + 1], ld, m.width, m.views_width, m.views_degree, view_dirs, pairs, u);
    SweepArgs a;
    a.acts = saved_acts; a.weights = weights; a.wvt = wvt; a.u = u; a.wo = params[pv + 2]; a.bo = params[pv + 3];
    a.products = products; a.total = total; a.blocks = (total + 31) / 32; a.num_rays = num_rays;
    a.samples = num_samples; a.views = num_views; a.act_rows = m.act_rows(); a.act_feature = m.act_feature();
    const dim3 grid((unsigned)((a.blocks + 3) / 4));
    if (m.wt == 8) hipLaunchKernelGGL((sweep_block_kernel<8, 4>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((sweep_block_kernel<4, 2>), grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(sweep_fold_kernel, dim3(snerf::stride_grid(pairs * 3, 256)), dim3(256), 0, s, products, acc, num_rays,
                       num_samples, num_views, white_bkgd ? 1 : 0, out_rgb);
    return snerf::check_launch("view_sweep");
}
