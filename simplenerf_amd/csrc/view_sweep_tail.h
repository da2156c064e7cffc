// What the view sweeps share around their matrix-core loop (view_sweep.hip: fp32 activations, view_sweep16.hip: 16-bit pieces):
// the pre-pass of the per-view direction term u, the per-view tail of a block's accumulator tiles, all fp32, and the sequential
// fold over a ray's samples.  Every operation and its order are those view_sweep.hip had when it owned this code (its operand
// format is the identity): its results are the same bits.
#pragma once
#include "mlp_device.h"
#include "mlp_layout.h"
#include "wave.h"

namespace {

long long round64(long long x) { return (x + 63) / 64 * 64; }

// The operand format of a sweep's products: fp32 as it is, or rounded to fp16 / bf16 (round to nearest even: the conversions
// mlp_pack.hip writes the 16-bit weight streams with and the 16-bit kernels convert their activations with) and widened again.
enum SweepFormat { kSweepFp32 = 0, kSweepF16 = 1, kSweepBf16 = 2 };
template <int FORMAT>
__device__ __forceinline__ float sweep_operand(float v) {
    if constexpr (FORMAT == kSweepF16) return (float)(_Float16)v;
    else if constexpr (FORMAT == kSweepBf16) return (float)(__bf16)v;
    else return v;
}

// u[v,n,:] = b_v + W_v[:, W:] . PE(d[v,n]).  One wave per (view, ray): the encoding in LDS (reference order: x, then sin / cos of
// every frequency), then two (Wv = 128) or one output feature per lane, e ascending.  Both factors in the sweep's operand format
// (a product of two 16-bit values is exact in fp32), the bias and the sum in fp32.
template <int FORMAT>
__global__ void __launch_bounds__(64) sweep_view_bias_kernel(const float* __restrict__ wv, const float* __restrict__ bv, int ld,
                                                             int width, int views_width, int degree,
                                                             const float* __restrict__ view_dirs, long long pairs,
                                                             float* __restrict__ u) {
    __shared__ float pe[3 + 6 * snerf::kMaxViewsDegree];
    const int lane = threadIdx.x;
    const int terms = 3 + 6 * degree;
    for (long long p = blockIdx.x; p < pairs; p += gridDim.x) {
        const float* d = view_dirs + 3 * p;
        if (lane < 3 * degree) {
            const int k = lane / 3, dim = lane - 3 * k;
            float s, c;
            sincos_turns((double)d[dim] * 0.15915494309189533576888 * (double)(1 << k), s, c);
            pe[3 + 6 * k + dim] = sweep_operand<FORMAT>(s);
            pe[6 + 6 * k + dim] = sweep_operand<FORMAT>(c);
        } else if (lane >= 32 && lane < 35) {
            pe[lane - 32] = sweep_operand<FORMAT>(d[lane - 32]);
        }
        snerf::wave_lds_sync();
        for (int j = lane; j < views_width; j += 64) {
            const float* row = wv + (long long)j * ld + width;
            float s = bv[j];
            for (int e = 0; e < terms; ++e) s = fmaf(sweep_operand<FORMAT>(row[e]), pe[e], s);
            u[p * views_width + j] = s;
        }
        snerf::wave_lds_sync();
    }
}

// `acc`: VT accumulator tiles of g for one 32-sample block, lane (j = lane & 31, h = lane >> 5) = sample j, register r of tile t =
// output feature 32 t + (r & 3) + 8 (r >> 2) + 4 h (mlp_layout.h): a lane half owns every other group of four features.
// `head`: LDS, W_o rows [3][WV] then b_o[3], 16-byte aligned.  `u`: [V][num_rays][WV].  Per view: relu(g + u), the 3 x WV head on the
// VALU with the cross-half add, the sigmoid, and weight * rgb of the lane's sample into products[v][c][sample].
template <int VT>
__device__ __forceinline__ void sweep_tail(const f32x16 (&acc)[VT], const float* head, const float* __restrict__ u,
                                           float* __restrict__ products, long long sample, bool live, long long ray, float weight,
                                           long long num_rays, long long total, int views, int h) {
    constexpr int WV = 32 * VT;
    const float b0 = head[3 * WV], b1 = head[3 * WV + 1], b2 = head[3 * WV + 2];
#pragma unroll 1
    for (int v = 0; v < views; ++v) {
        asm volatile("" ::: "memory");      // the head weights are read from LDS per view, not hoisted into 3 x Wv / 2 registers
        const float* uv = u + ((long long)v * num_rays + ray) * WV + 4 * h;
        float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
#pragma unroll
        for (int t = 0; t < VT; ++t) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int f = 32 * t + 8 * g;       // + 4 h: in the pointers
                const f32x4 uu = *reinterpret_cast<const f32x4*>(uv + f);
                const f32x4 w0 = *reinterpret_cast<const f32x4*>(head + 4 * h + f);
                const f32x4 w1 = *reinterpret_cast<const f32x4*>(head + WV + 4 * h + f);
                const f32x4 w2 = *reinterpret_cast<const f32x4*>(head + 2 * WV + 4 * h + f);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float x = fmaxf(acc[t][4 * g + q] + uu[q], 0.0f);
                    p0 = fmaf(w0[q], x, p0);
                    p1 = fmaf(w1[q], x, p1);
                    p2 = fmaf(w2[q], x, p2);
                }
            }
        }
        p0 += __shfl_xor(p0, 32, 64);
        p1 += __shfl_xor(p1, 32, 64);
        p2 += __shfl_xor(p2, 32, 64);
        if (live && h == 0) {
            float* out = products + (long long)v * 3 * total + sample;
            out[0] = weight * sigmoidf(p0 + b0);
            out[total] = weight * sigmoidf(p1 + b1);
            out[2 * total] = weight * sigmoidf(p2 + b2);
        }
    }
}

// out[v,n,c] = the samples' products summed s = 0 .. S-1 by one thread: a fixed order that does not depend on how the ray's samples
// fall into the 32-sample blocks
__global__ void __launch_bounds__(256) sweep_fold_kernel(const float* __restrict__ products, const float* __restrict__ acc,
                                                         long long num_rays, int samples, int views, int white_bkgd,
                                                         float* __restrict__ out) {
    const long long count = (long long)views * 3 * num_rays, total = num_rays * samples;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < count; t += (long long)gridDim.x * 256) {
        const long long vc = t / num_rays, ray = t - vc * num_rays;
        const float* p = products + vc * total + ray * samples;
        float sum = 0.0f;
        for (int s = 0; s < samples; ++s) sum += p[s];
        if (white_bkgd) sum += 1.0f - acc[ray];
        const long long v = vc / 3;
        out[(v * num_rays + ray) * 3 + (vc - 3 * v)] = sum;
    }
}

}  // namespace
