// The last product of the fp32 backward chain, which training never needed: the gradient with respect to the MLP's input point
// (simplenerf_gradient.h has the rule).  The chain (mlp_backward.hip, B1) has written every dY_l as [feature][32-sample] tiles;
// this kernel forms, per 32-sample wave block,
//   d enc^T[64, 32] = W_0^T . dY_0^T (+ W_5[:, :pts_in]^T . dY_5^T through the skip connection)
// on the fp32 matrix cores (v_mfma_f32_32x32x2_f32; pts_in <= 63 rows padded with zero rows to two 32-row tiles) and applies the
// positional encoding's Jacobian with the sines and cosines the training forward saved.
//
// Operands.  A = W^T: the reference-layout weights (out, in) row-major are staged ONCE per workgroup in LDS in fragment order --
//   float ((ks4 . 2 + t) . 64 + lane) . 4 + q  =  W[f = 2 (4 ks4 + q) + (lane >> 5)][e = 32 t + (lane & 31)], 0 for e >= pts_in --
//   so that a lane reads the four k-steps of a tile with one 16-byte LDS read at a 16-byte lane stride (conflict-free).  At most
//   2 x 256 x 64 floats = 128 KiB.  B = dY^T: lane (j, half) of k-step ks reads tile[(2 ks + half) . 32 + j], 256 contiguous bytes
//   per wave and k-step, straight from the chain's workspace.  D: register r of lane (j, half) of tile t is encoding feature
//   32 t + (r & 3) + 8 (r >> 2) + 4 half of sample j (store_acc_tile's layout, mlp_device.h).
// A workgroup of four waves walks wave blocks with a grid stride, one per wave and round; nothing is shared after the staging, so
// no barrier follows it.  One owner per output element, a fixed order of sums, no atomics.
// Bound: the dY_0 / dY_5 tiles are read once (2 KiB a sample at width 256) for 2 x 2 x 64 x width FLOP a sample, about 1/9 of the
// trunk's; L2 / HBM-bound beside the chain.
#include "mlp_device.h"

namespace snerf {

struct InputGradArgs {
    const float* w0;        // pts_linears.0.weight (width, pts_in)
    const float* w5;        // pts_linears.5.weight (width, pts_in + width), or NULL without a skip layer
    const float* acts;      // saved activation tiles (the encoding rows are read)
    const float* grads;     // the chain's dY tiles
    float* d_points;        // (total, 3)
    long long total;
    long long wave_blocks;  // ceil(total / 32)
    int pts_in, act_rows, grad_rows, grad_y5;
};

namespace {

template <int WIDTH>
__global__ void __launch_bounds__(256) mlp_input_grad_kernel(InputGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int kOperandFloats = WIDTH * 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, half = lane >> 5;
    const int operands = a.w5 ? 2 : 1;
    for (int op = 0; op < operands; ++op) {
        const float* w = op ? a.w5 : a.w0;
        const int ld = op ? a.pts_in + WIDTH : a.pts_in;
        for (int at = threadIdx.x; at < kOperandFloats; at += 256) {
            const int e = at & 63, f = at >> 6;          // (e fastest: rows of the source are read contiguously)
            const int ks = f >> 1;
            const float v = e < a.pts_in ? w[(long long)f * ld + e] : 0.0f;
            lds[op * kOperandFloats + ((((ks >> 2) * 2 + (e >> 5)) * 64 + (f & 1) * 32 + (e & 31)) << 2) + (ks & 3)] = v;
        }
    }
    __syncthreads();

    for (long long block = (long long)blockIdx.x * 4 + wave; block < a.wave_blocks; block += (long long)gridDim.x * 4) {
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        for (int op = 0; op < operands; ++op) {
            const float* tile = a.grads + (block * a.grad_rows + (op ? a.grad_y5 : 0)) * 32 + lane;
            const float* frag = lds + op * kOperandFloats + lane * 4;
#pragma unroll 4
            for (int ks4 = 0; ks4 < WIDTH / 8; ++ks4) {
                float b[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) b[q] = tile[(4 * ks4 + q) * 64];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(frag + (ks4 * 2 + t) * 256);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[q], b[q], acc[t], 0, 0, 0);
                }
            }
        }
        // the encoding's Jacobian: this lane holds 32 of its sample's 64 encoding features, in ascending order
        const float* pe = a.acts + block * a.act_rows * 32 + j;
        double g0 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int e = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (e >= a.pts_in) continue;
                double term = (double)acc[t][r];
                if (e >= 3) {
                    const int m = e - 3, k = m / 6, rem = m - 6 * k;
                    const bool is_cos = rem >= 3;
                    const double other = (double)pe[(is_cos ? e - 3 : e + 3) * 32];    // cos row of a sin feature, sin row of a cos one
                    term = (double)(1 << k) * (other * term);
                    if (is_cos) term = -term;
                }
                const int axis = e % 3;
                g0 += axis == 0 ? term : 0.0;
                g1 += axis == 1 ? term : 0.0;
                g2 += axis == 2 ? term : 0.0;
            }
        }
        g0 += __shfl_xor(g0, 32, 64);
        g1 += __shfl_xor(g1, 32, 64);
        g2 += __shfl_xor(g2, 32, 64);
        const long long sample = block * 32 + j;
        if (half == 0 && sample < a.total) {
            a.d_points[3 * sample + 0] = (float)g0;
            a.d_points[3 * sample + 1] = (float)g1;
            a.d_points[3 * sample + 2] = (float)g2;
        }
    }
}

template <int WIDTH>
int launch(const InputGradArgs& a, hipStream_t stream) {
    const int lds_bytes = (a.w5 ? 2 : 1) * WIDTH * 64 * (int)sizeof(float);
    auto kernel = mlp_input_grad_kernel<WIDTH>;
    static DeviceOnce configured;   // per device: the attribute belongs to (kernel, device)
    const int attr = raise_dynamic_lds(configured, reinterpret_cast<const void*>(kernel), 2 * WIDTH * 64 * (int)sizeof(float), "mlp_input_gradient");
    if (attr != SNERF_OK) return attr;
    // one workgroup per CU at most (128 KiB of LDS at width 256): the staging is paid once per workgroup
    const long long wanted = (a.wave_blocks + 3) / 4;
    const long long cap = persistent_workgroups() / 2 > 0 ? persistent_workgroups() / 2 : 1;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(wanted < cap ? wanted : cap)), dim3(256), lds_bytes, stream, a);
    return check_launch("mlp_input_gradient(encoding)");
}

}  // namespace

// width: 128 or 256 (the fused shapes); the caller has checked every limit
int mlp_input_gradient_encoding(const MlpPlan& plan, const float* w0, const float* w5, const float* acts, const float* grads,
                                long long total, float* d_points, hipStream_t stream) {
    InputGradArgs a;
    a.w0 = w0; a.w5 = w5; a.acts = acts; a.grads = grads; a.d_points = d_points;
    a.total = total; a.wave_blocks = (total + 31) / 32;
    a.pts_in = plan.pts_in; a.act_rows = plan.act_rows(); a.grad_rows = plan.grad_rows(); a.grad_y5 = plan.grad_y(5);
    if (plan.width == 256) return launch<256>(a, stream);
    if (plan.width == 128) return launch<128>(a, stream);
    return fail(SNERF_E_UNSUPPORTED, "mlp_input_gradient: points_net_width %d not built (128 or 256)", plan.width);
}

}  // namespace snerf
