// Kernels of the layered MLP path that do not depend on the GEMM's operand precision: the encoding, the heads, the
// fixed-order split reductions and bias sums, shared by the fp32 path (mlp_generic.hip) and its bf16-operand variant
// (mlp_generic_bf16.hip).  Every definition sits in an unnamed namespace: each translation unit has its own copy.
#pragma once
#include "mlp_device.h"

namespace {

// a value as the activation matrix holds it: fp32, or bf16 bits (round to nearest even)
template <typename T> __device__ __forceinline__ T store_as(float v);
template <> __device__ __forceinline__ float store_as<float>(float v) { return v; }
template <> __device__ __forceinline__ unsigned short store_as<unsigned short>(float v) {
    return __builtin_bit_cast(unsigned short, (__bf16)v);
}

// ------------------------------------------------------------------------------------------------------ encoding + heads
// [x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ...] (PositionalEncoder :533-557) with the fused kernels' exact range reduction
struct EncodeArgs {
    const float *origins, *dirs, *view_dirs, *depths;
    void* acts; long long row;                           // float (fp32 path) or bf16 bits (bf16 path)
    long long total; int samples;
    int points_degree, views_degree, pe_full, pts_in, views_pe;
    int c_pe, c_pev, c_x5, c_v0_extra, c_v0_views;       // -1 = block absent
};

// One thread per (sample, destination column): neighbouring lanes write neighbouring columns of one row.  (Round 4's kernel gave a
// thread a whole sample: every store of a wave went to 64 different rows -- 0.62 ms of the 8 x 512 forward at 262 144 samples,
// profiles/r05_layered_kernel_stats.csv.  The copies of the encoding a layer input needs -- skip layer, views layer -- are computed
// again instead of read back: same function of the same inputs, same bits.)
__device__ __forceinline__ float encode_column(const float (&x)[3], int c) {
    constexpr double kInvTwoPi = 0.15915494309189533576888;
    if (c < 3) return x[c];
    const int k = (c - 3) / 6, r = (c - 3) % 6, d = r % 3;
    float sn, cs;
    sincos_turns((double)x[d] * kInvTwoPi * (double)(1 << k), sn, cs);
    return r < 3 ? sn : cs;
}

template <typename T>
__global__ void __launch_bounds__(256) encode_kernel(EncodeArgs a) {
    // destination blocks of a row, in order: [encoding | its first pts_in columns for the skip layer | its remaining columns for the
    // views layer | view encoding | view encoding for the views layer]
    const int n_pe = a.pe_full, n_x5 = a.c_x5 >= 0 ? a.pts_in : 0, n_extra = a.c_v0_extra >= 0 ? a.pe_full - a.pts_in : 0;
    const int n_pev = a.views_pe > 0 ? a.views_pe : 0;
    const int width = n_pe + n_x5 + n_extra + 2 * n_pev;
    const long long count = a.total * width, stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += stride) {
        const long long s = e / width;
        int j = (int)(e - s * width);
        const long long ray = s / a.samples;
        T* row = static_cast<T*>(a.acts) + s * a.row;
        int dest, c;
        bool views = false;
        if (j < n_pe) { dest = a.c_pe + j; c = j; }
        else if ((j -= n_pe) < n_x5) { dest = a.c_x5 + j; c = j; }
        else if ((j -= n_x5) < n_extra) { dest = a.c_v0_extra + j; c = a.pts_in + j; }
        else if ((j -= n_extra) < n_pev) { dest = a.c_pev + j; c = j; views = true; }
        else { j -= n_pev; dest = a.c_v0_views + j; c = j; views = true; }
        float x[3];
        if (views) {
            for (int k = 0; k < 3; ++k) x[k] = a.view_dirs[ray * 3 + k];
        } else {
            const float z = a.depths[s];
            for (int k = 0; k < 3; ++k) x[k] = a.origins[ray * 3 + k] + a.dirs[ray * 3 + k] * z;   // mul, then add (:140-142)
        }
        row[dest] = store_as<T>(encode_column(x, c));
    }
}

// pts_output / views_output rows -> sigma (N), rgb (N,3) (:664-681, :703-706)
__global__ void __launch_bounds__(256) heads_kernel(const float* __restrict__ acts, long long row, int c_out, int c_vout, int view_dep,
                                                    const float* __restrict__ noise, long long total, float* __restrict__ sigma,
                                                    float* __restrict__ rgb) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < total; s += stride) {
        const float* r = acts + s * row;
        float sg = r[c_out];
        if (noise) sg += noise[s];
        sigma[s] = fmaxf(sg, 0.0f);
        const float* col = view_dep ? r + c_vout : r + c_out + 1;
        for (int c = 0; c < 3; ++c) rgb[s * 3 + c] = sigmoidf(col[c]);
    }
}

// d sigma, d rgb -> gradients of the two head pre-activations: dout (N,4) and dvout (N,4), zero-padded
__global__ void __launch_bounds__(256) heads_backward_kernel(const float* __restrict__ sigma, const float* __restrict__ rgb,
                                                             const float* __restrict__ d_sigma, const float* __restrict__ d_rgb,
                                                             long long total, int view_dep, float* __restrict__ dout,
                                                             float* __restrict__ dvout) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < total; s += stride) {
        float col[3];
        for (int c = 0; c < 3; ++c) {
            const float v = rgb[s * 3 + c];
            col[c] = d_rgb[s * 3 + c] * (v * (1.0f - v));
        }
        dout[s * 4] = sigma[s] > 0.0f ? d_sigma[s] : 0.0f;
        for (int c = 0; c < 3; ++c) {
            dout[s * 4 + 1 + c] = view_dep ? 0.0f : col[c];
            if (view_dep) dvout[s * 4 + c] = col[c];
        }
        if (view_dep) dvout[s * 4 + 3] = 0.0f;
    }
}

// out[m][n] (+)= sum_z partial[z][m][n] in z order (bit-reproducible).  The partials are summed first and the sum added to what
// `out` holds once: accumulating equals prior + fresh in one rounding (starting the chain from the prior lost its low bits wherever
// the partials cancel: 4.5 fp32 ulps of max(|prior|, |fresh|) in a bias gradient, tests/test_gpu_rounding.py)
__global__ void __launch_bounds__(256) reduce_splits_kernel(const float* __restrict__ partial, long long split_stride, int splits,
                                                            long long count, float* __restrict__ out, int accumulate) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += stride) {
        float s = 0.0f;
        for (int z = 0; z < splits; ++z) s += partial[z * split_stride + e];
        out[e] = accumulate ? out[e] + s : s;
    }
}

// column sums of dZ (N x cols, row stride ld) over a chunk of rows: partial[z][col]
__global__ void __launch_bounds__(256) colsum_kernel(const float* __restrict__ dz, long long ld, long long rows, int cols,
                                                     long long rows_per_split, float* __restrict__ partial) {
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
    const long long lo = (long long)blockIdx.y * rows_per_split, hi = lo + rows_per_split < rows ? lo + rows_per_split : rows;
    float s = 0.0f;
    if (col < cols)
        for (long long r = lo + part; r < hi; r += 4) s += dz[r * ld + col];
    __shared__ float sh[4][64];
    sh[part][threadIdx.x & 63] = s;
    __syncthreads();
    if (part == 0 && col < cols) partial[(long long)blockIdx.y * cols + col] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

}  // namespace
