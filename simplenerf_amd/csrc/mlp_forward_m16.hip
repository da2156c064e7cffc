// K3 (fp16 modes, inference) on v_mfma_f32_16x16x32_f16 -- the same fused PE + MLP forward as mlp_forward_f16.hip, same
// arithmetic per product (P = 3: hi.hi + hi.lo + lo.hi; P = 1: hi.hi), same unit stream mechanics, different MFMA shape.
//
// Why a second shape.  Every fp16-mode kernel runs the board at its 1400 W cap, so what counts is work per
// joule.  Bare loops over the same data (tools/probes/mfma_shape_power.hip: fragment from LDS, operands in registers,
// accumulation as here) deliver 1.55 PFLOP/s with v_mfma_f32_32x32x16_f16 and 1.70 PFLOP/s with v_mfma_f32_16x16x32_f16 at
// the same 1355 W and the same 2.3 GHz: four independent 16-cycle accumulator chains keep the pipe fuller than one
// 32-cycle chain.  The training kernels stay on the 32x32x16 layout their saved tensors are written in.
//
// Layout.  A wave still owns 32 samples and accumulates one 32-row out tile over all its k-steps before the next; the
// tile is four 16x16 accumulators acc[r][s] (row half r, sample half s; lane (n = lane & 15, g = lane >> 4) holds rows
// 16r + 4g .. +3 of sample 16s + n).  A 1-KiB weight fragment is 16 out rows x 32 inputs (k-block c, row half r) and feeds
// two MFMAs, one per sample half.  The B operand of k-block c of the NEXT layer is, per lane, {acc[0][s] (4 values),
// acc[1][s] (4 values)} of out tile c -- again no data movement between layers; mlp_pack.hip orders the weights' k slots
// to match (MlpPlan::m16_stages).  The encodings are computed in the 32x32 lane mapping (one sample per lane, no
// redundancy) and redistributed once through LDS.
//
// Built for the view-dependent 8 x 256 main MLP (what rendering evaluates); everything else takes mlp_forward_f16.hip.
// Bound: MFMA fp16 under the board power cap.

#include "mlp_forward_m16_body.h"

namespace {

template <int P, int DEPTH, bool BF = false>
__global__ void __launch_bounds__(P == 1 ? 512 : 256, P == 1 ? 2 : 1) mlp_forward_m16_kernel(M16Args args) {
    mlp_forward_m16_body<P, DEPTH, BF>(args, blockIdx.x);
}

template <int P, bool BF = false>
int launch_m16(const M16Args& args, hipStream_t stream) {
    constexpr int NW = P == 1 ? 8 : 4;
    const long long blocks = (args.m.total + NW * 32 - 1) / (NW * 32);
    if (blocks > 0x7fffffffLL) return snerf::fail(SNERF_E_UNSUPPORTED, "mlp_forward: too many samples in one call");
    constexpr int RING = m16_ring(P);
    // the encodings' scratch (NW x 6 KiB) lies in the ring's slots from the third on
    if ((size_t)(RING - 2) * args.slot_floats < (size_t)NW * 6 * 256)
        return snerf::fail(SNERF_E_UNSUPPORTED, "mlp_forward(m16): ring slots of %d floats cannot hold the encoding scratch", args.slot_floats);
    const size_t lds_bytes = sizeof(float) * m16_lds_floats(P, args);
    auto kernel = mlp_forward_m16_kernel<P, 8, BF>;
    static snerf::DeviceOnce configured;   // per device: the attribute belongs to (kernel, device)
    const int attr = snerf::raise_dynamic_lds(configured, reinterpret_cast<const void*>(kernel), (int)(sizeof(float) * (kUnitBuffers * kUnitBufFloats + 2048 + 5120)), "mlp_forward");   // (P = 3: 132 + 8 + 20 KiB; P = 1: 4 x 24 + 8 + 20 KiB)
    if (attr != SNERF_OK) return attr;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(NW * 64), lds_bytes, stream, args);
    return snerf::check_launch("mlp_forward(m16)");
}

}  // namespace

namespace snerf {

// Inference with the fp16 modes for the layout this file builds; -1 = the caller uses mlp_forward_f16.hip.
// `bf16`: the single-product kernel on bf16 operands (SNERF_PRECISION_BF16), reading the compact bf16 copy of the stream.
int mlp_forward_m16(const MlpPlan& plan, const MlpArgs& m, int products, hipStream_t stream, bool bf16) {
    M16Args args;
    if (!m16_args_of(plan, m, products, bf16, &args)) return -1;
    if (bf16) return launch_m16<1, true>(args, stream);
    return products == 3 ? launch_m16<3>(args, stream) : launch_m16<1>(args, stream);
}

}  // namespace snerf
