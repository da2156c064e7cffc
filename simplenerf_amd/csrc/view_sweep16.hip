// snerf_view_sweep_half (simplenerf_sweep16.h): the view sweep of a model that renders at SNERF_PRECISION_F16 / _BF16, from the
// `feature` pieces a storing 16-bit forward has left in the saved activations.  Four launches, all in stream order:
//   1. sweep16_operand_kernel   r(W_v[:, :W]) -> the workspace as A operand fragments [k-step][out tile][lane][8 x 16 bit]
//   2. sweep_view_bias_kernel   (view_sweep_tail.h) u[v,n,:] = b_v + r(W_v[:, W:]) . r(PE(d[v,n])), one wave per (view, ray)
//   3. sweep16_block_kernel     one wave per 32-sample block: g = r(W_v[:, :W]) . feature16 on v_mfma_f32_32x32x16_{f16,bf16} -- a
//                               lane's 16 bytes of a saved piece ARE its B operand -- into the accumulator tiles of the fp32
//                               sweep, then the same fp32 tail over the views (sweep_tail)
//   4. sweep_fold_kernel        (view_sweep_tail.h) the sequential sum over a ray's samples
// DESIGN.md section 9 has the reasons for each choice and the measured numbers.
#include "mlp_device_f16.h"
#include "mlp_plan.h"
#include "simplenerf_sweep16.h"
#include "view_sweep_tail.h"

namespace {

struct Sweep16Args {
    const _Float16* acts;     // saved activations, rows of 32 x 16 bit: [block][act16_rows][32]
    const float* weights;     // (total)
    const f16x8* wva;         // workspace: [W / 16][VT][64 lanes] fragments
    const float* u;           // workspace: [V][n][Wv]
    const float* wo;          // views_output_linear.weight (3, Wv)
    const float* bo;          // views_output_linear.bias (3)
    float* products;          // workspace: [V][3][total]
    long long total, blocks, num_rays;
    int samples, views, act_rows, act_feature;
};

// One thread per 16-bit element: fragment (ks, t), lane (j, h), element e <- r(W_v[32 t + j][16 ks + 8 (e >> 2) + 4 h + (e & 3)]),
// the feature a saved piece holds in element e of the same lane half (store_pieces, mlp_device_f16.h).  The rounding is
// pack_half_stage_kernel's (mlp_pack.hip): a plain conversion, round to nearest even.
template <bool BF>
__global__ void __launch_bounds__(256) sweep16_operand_kernel(const float* __restrict__ wv, int ld, int width, int views_width,
                                                              _Float16* __restrict__ wva) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= width * views_width) return;
    const int e = idx & 7, lane = (idx >> 3) & 63, frag = idx >> 9;
    const int vt = views_width / 32, t = frag % vt, ks = frag / vt;
    const int row = 32 * t + (lane & 31), col = 16 * ks + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
    wva[idx] = pack_one<BF>(wv[(long long)row * ld + col]);
}

// Four waves per workgroup, one 32-sample block each, as sweep_block_kernel (view_sweep.hip); W / 16 k-steps of VT MFMAs.  Per
// k-step a wave reads one KiB of its block's pieces and VT KiB of the operand fragments (64 KB in all: they stay in L2).
// At least two waves per SIMD (launch bounds): a single wave has nobody to hide the loads of the matrix-core loop behind.
template <int WT, int VT, bool BF>
__global__ void __launch_bounds__(256, 2) sweep16_block_kernel(Sweep16Args a) {
    constexpr int KS = 2 * WT, WV = 32 * VT;
    __shared__ __attribute__((aligned(16))) float head[3 * WV + 4];
    for (int i = threadIdx.x; i < 3 * WV + 3; i += 256) head[i] = i < 3 * WV ? a.wo[i] : a.bo[i - 3 * WV];
    __syncthreads();
    const long long block = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (block >= a.blocks) return;          // (whole waves)
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;

    // the lane's slot of piece ks: 2 j + h (16 bytes); a piece is 512 elements
    const f16x8* feat = reinterpret_cast<const f16x8*>(a.acts + (block * a.act_rows + a.act_feature) * 32) + 2 * j + h;
    const f16x8* wfrag = a.wva + lane;
    f32x16 acc[VT];
#pragma unroll
    for (int t = 0; t < VT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
#pragma unroll 4
    for (int ks = 0; ks < KS; ++ks) {
        const f16x8 b = __builtin_nontemporal_load(feat + ks * 64);      // read once
#pragma unroll
        for (int t = 0; t < VT; ++t) acc[t] = mfma_32x32x16<BF>(wfrag[(ks * VT + t) * 64], b, acc[t]);
    }

    // the lane's sample: a block may hold samples of several rays, and the last block of a call is partial
    const long long sample = block * 32 + j;
    const bool live = sample < a.total;
    const long long ray = live ? sample / a.samples : a.num_rays - 1;
    const float weight = live ? a.weights[sample] : 0.0f;
    sweep_tail<VT>(acc, head, a.u, a.products, sample, live, ray, weight, a.num_rays, a.total, a.views, h);
}

struct Sweep16Plan {
    snerf::MlpPlan mlp;
    long long blocks = 0, acts_floats = 0;
    long long wva_floats = 0, u_floats = 0, product_floats = 0;
    long long total() const { return wva_floats + u_floats + product_floats; }
};

// !views_given: the query of what the call reads of saved_acts, which does not depend on the views
int plan_sweep16(const snerf_mlp_desc* desc, long long num_rays, int num_samples, int num_views, bool views_given, Sweep16Plan* out) {
    if (!desc) return snerf::fail(SNERF_E_INVALID, "view_sweep_half: NULL descriptor");
    Sweep16Plan p;
    const int st = snerf::build_plan(desc, &p.mlp);
    if (st == SNERF_E_UNSUPPORTED)
        return snerf::fail(SNERF_E_UNSUPPORTED, "view_sweep_half: built for the fused 16-bit layouts only (points_net_width / views_net_width "
                           "256 / 128 or 128 / 64, views_net_depth 1), not for a layered shape (width %d, views depth %d, views width %d)",
                           desc->points_net_width, desc->views_net_depth, desc->views_net_width);
    if (st != SNERF_OK) return st;
    const snerf::MlpPlan& m = p.mlp;
    if (!m.view_dependent)
        return snerf::fail(SNERF_E_UNSUPPORTED, "view_sweep_half: the MLP has no views head (view_dependent_rgb = 0): its colour does not "
                           "depend on the view direction");
    if (m.sigma_pe)
        return snerf::fail(SNERF_E_UNSUPPORTED, "view_sweep_half: sigma_pe_degree %d not built (-1): the views layer of a "
                           "points-augmentation layout also reads the point encoding", desc->sigma_pe_degree);
    if (desc->predict_visibility)
        return snerf::fail(SNERF_E_UNSUPPORTED, "view_sweep_half: predict_visibility MLPs are not built");
    if (!((m.width == 256 && m.views_width == 128) || (m.width == 128 && m.views_width == 64)))
        return snerf::fail(SNERF_E_UNSUPPORTED, "view_sweep_half: points_net_width / views_net_width %d / %d not built (256 / 128 or "
                           "128 / 64)", m.width, m.views_width);
    SNERF_REQUIRE(num_rays >= 0, "view_sweep_half: num_rays %lld < 0", num_rays);
    SNERF_REQUIRE(num_samples >= 1, "view_sweep_half: num_samples %d < 1", num_samples);
    SNERF_REQUIRE(!views_given || num_views >= 0, "view_sweep_half: num_views %d < 0", num_views);
    SNERF_REQUIRE(num_rays <= (1ll << 40) / num_samples, "view_sweep_half: %lld rays x %d samples: too many samples for one call",
                  num_rays, num_samples);
    p.blocks = (num_rays * num_samples + 31) / 32;
    // rows of 32 x 16 bit = 16 floats: every block before the last one whole, the last one up to the end of its feature rows
    p.acts_floats = p.blocks ? ((p.blocks - 1) * m.act16_rows() + m.act_feature() + m.width) * 16 : 0;
    if (views_given) {
        p.wva_floats = (long long)m.width * m.views_width / 2;
        p.u_floats = round64((long long)num_views * num_rays * m.views_width);
        p.product_floats = round64((long long)num_views * 3 * num_rays * num_samples);
    }
    *out = p;
    return SNERF_OK;
}

}  // namespace

extern "C" size_t snerf_view_sweep_half_workspace_floats(const snerf_mlp_desc* desc, long long num_rays, int num_samples,
                                                         int num_views) {
    Sweep16Plan p;
    if (plan_sweep16(desc, num_rays, num_samples, num_views, true, &p) != SNERF_OK) return 0;
    return (size_t)p.total();
}

extern "C" size_t snerf_view_sweep_half_acts_floats(const snerf_mlp_desc* desc, long long num_rays, int num_samples) {
    Sweep16Plan p;
    if (plan_sweep16(desc, num_rays, num_samples, 0, false, &p) != SNERF_OK) return 0;
    return (size_t)p.acts_floats;
}

extern "C" int snerf_view_sweep_half(const snerf_mlp_desc* desc, const float* const* params, int num_params, const float* saved_acts,
                                     const float* weights, const float* acc, const float* view_dirs, long long num_rays,
                                     int num_samples, int num_views, int white_bkgd, int precision, float* out_rgb, float* workspace,
                                     snerf_stream_t stream) {
    Sweep16Plan p;
    const int st = plan_sweep16(desc, num_rays, num_samples, num_views, true, &p);
    if (st != SNERF_OK) return st;
    const snerf::MlpPlan& m = p.mlp;
    SNERF_REQUIRE(precision == SNERF_PRECISION_F16 || precision == SNERF_PRECISION_BF16,
                  "view_sweep_half: precision %d: reads the 16-bit pieces of SNERF_PRECISION_F16 (%d) or SNERF_PRECISION_BF16 (%d) -- "
                  "snerf_view_sweep reads fp32 activations", precision, (int)SNERF_PRECISION_F16, (int)SNERF_PRECISION_BF16);
    if (num_rays == 0 || num_views == 0) return SNERF_OK;
    SNERF_REQUIRE(params, "view_sweep_half: NULL params");
    SNERF_REQUIRE(num_params == m.num_params, "view_sweep_half: %d parameter tensors, the descriptor has %d", num_params, m.num_params);
    const int pv = 2 * m.depth + 4;       // views_linears.0.weight, .bias, views_output_linear.weight, .bias
    for (int i = pv; i < pv + 4; ++i) SNERF_REQUIRE(params[i], "view_sweep_half: params[%d] is NULL", i);
    SNERF_REQUIRE(!white_bkgd || acc, "view_sweep_half: white_bkgd needs acc (NULL)");
    SNERF_REQUIRE(saved_acts && weights && view_dirs && out_rgb && workspace, "view_sweep_half: NULL pointer (saved_acts, weights, "
                  "view_dirs, out_rgb or workspace)");
    SNERF_REQUIRE(((unsigned long long)workspace & 15) == 0, "view_sweep_half: workspace must be 16-byte aligned");
    SNERF_REQUIRE(((unsigned long long)saved_acts & 15) == 0, "view_sweep_half: saved_acts must be 16-byte aligned");
    const long long total = num_rays * num_samples, pairs = (long long)num_views * num_rays;
    SNERF_REQUIRE(pairs * 3 < (1ll << 40), "view_sweep_half: %d views x %lld rays: too many for one call", num_views, num_rays);
    SNERF_REQUIRE((p.blocks + 3) / 4 <= 0x7fffffffLL, "view_sweep_half: %lld sample blocks: too many for one call", p.blocks);
    hipStream_t s = (hipStream_t)stream;
    const int ld = m.width + m.views_pe;
    const bool bf = precision == SNERF_PRECISION_BF16;
    float* wva = workspace;
    float* u = wva + p.wva_floats;
    float* products = u + p.u_floats;

    const dim3 operand_grid((unsigned)((m.width * m.views_width + 255) / 256)), bias_grid((unsigned)(pairs < 65536 ? pairs : 65536));
    if (bf) {
        hipLaunchKernelGGL(sweep16_operand_kernel<true>, operand_grid, dim3(256), 0, s, params[pv], ld, m.width, m.views_width,
                           reinterpret_cast<_Float16*>(wva));
        hipLaunchKernelGGL(sweep_view_bias_kernel<kSweepBf16>, bias_grid, dim3(64), 0, s, params[pv], params[pv + 1], ld, m.width,
                           m.views_width, m.views_degree, view_dirs, pairs, u);
    } else {
        hipLaunchKernelGGL(sweep16_operand_kernel<false>, operand_grid, dim3(256), 0, s, params[pv], ld, m.width, m.views_width,
                           reinterpret_cast<_Float16*>(wva));
        hipLaunchKernelGGL(sweep_view_bias_kernel<kSweepF16>, bias_grid, dim3(64), 0, s, params[pv], params[pv + 1], ld, m.width,
                           m.views_width, m.views_degree, view_dirs, pairs, u);
    }
    Sweep16Args a;
    a.acts = reinterpret_cast<const _Float16*>(saved_acts); a.weights = weights; a.wva = reinterpret_cast<const f16x8*>(wva); a.u = u;
    a.wo = params[pv + 2]; a.bo = params[pv + 3]; a.products = products; a.total = total; a.blocks = p.blocks; a.num_rays = num_rays;
    a.samples = num_samples; a.views = num_views; a.act_rows = m.act16_rows(); a.act_feature = m.act_feature();
    const dim3 grid((unsigned)((a.blocks + 3) / 4));
    if (m.wt == 8) {
        if (bf) hipLaunchKernelGGL((sweep16_block_kernel<8, 4, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((sweep16_block_kernel<8, 4, false>), grid, dim3(256), 0, s, a);
    } else {
        if (bf) hipLaunchKernelGGL((sweep16_block_kernel<4, 2, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((sweep16_block_kernel<4, 2, false>), grid, dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(sweep_fold_kernel, dim3(snerf::stride_grid(pairs * 3, 256)), dim3(256), 0, s, products, acc, num_rays,
                       num_samples, num_views, white_bkgd ? 1 : 0, out_rgb);
    return snerf::check_launch("view_sweep_half");
}
