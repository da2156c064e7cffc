// The workgroup reduction of the metric kernels (csrc/metrics.hip, csrc/lpips.hip): thread -> wave (xor shuffles) -> workgroup
// (LDS, wave order).  Fixed order, no atomics: the same input gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace snerf {
namespace reduce {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

template <typename T>
__device__ __forceinline__ T wave_sum_t(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Sum of `v` over the workgroup's kBlock threads, valid in thread 0.  `lds` holds kWaves values; reusable after the call.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* lds) {
    v = wave_sum_t(v);
    __syncthreads();   // (the previous use of `lds` has been read)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += lds[w];
    return s;
}

// The same walk for any associative, commutative `op` (e.g. a maximum): valid in EVERY thread.
template <typename T, typename Op>
__device__ __forceinline__ T block_fold(T v, T* lds, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s = op(s, lds[w]);
    return s;
}

}  // namespace reduce
}  // namespace snerf
