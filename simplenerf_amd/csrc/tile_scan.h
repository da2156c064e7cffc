// Count per tile, scan, scatter: the workgroup scans and tile ranks that the order-preserving compactions of fuse.hip and mesh.hip
// share, on the tiling of sort_plan.h (a tile is kTile consecutive positions; wave, round, lane IS the index order).  Device code only;
// every function is local to the translation unit that includes it.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "sort_plan.h"

namespace snerf {
namespace tilescan {

using namespace snerf::sortplan;

static __device__ __forceinline__ uint32_t wave_inclusive_add_u32(uint32_t v) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t n = __shfl_up(v, off, kWave);
        if (lane >= off) v += n;
    }
    return v;
}

// Exclusive scan of `v` over the workgroup in thread order; *total receives the workgroup's sum.  `lds` holds kWaves values.
static __device__ __forceinline__ uint32_t block_exclusive_add(uint32_t v, uint32_t* lds, uint32_t* total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t inclusive = wave_inclusive_add_u32(v);
    __syncthreads();
    if (lane == kWave - 1) lds[wave] = inclusive;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        if (k < wave) before += lds[k];
        all += lds[k];
    }
    *total = all;
    return before + inclusive - v;
}

// grid (1): counters[0 .. n) scanned exclusively in place, a chunk of kScanChunk at a time, the carry kept by every thread
static __global__ void __launch_bounds__(kBlock) scan_counters_kernel(uint32_t* __restrict__ counters, long long n) {
    __shared__ uint32_t lds[kWaves];
    uint32_t carry = 0;
    for (long long chunk = 0; chunk < n; chunk += kScanChunk) {
        const long long first = chunk + (long long)threadIdx.x * kScanItems;
        uint32_t item[kScanItems], mine = 0;
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            item[j] = first + j < n ? counters[first + j] : 0u;
            mine += item[j];
        }
        uint32_t total;
        uint32_t running = carry + block_exclusive_add(mine, lds, &total);
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            if (first + j < n) counters[first + j] = running;
            running += item[j];
        }
        carry += total;
    }
}

// The positions inside the tile of the calling thread's kept rounds (bit r of `kept`): rank[r] counts the kept positions before it in
// its wave; *start receives what the lower waves keep, *all the tile's total.  wave_total: kWaves values in LDS.
static __device__ __forceinline__ void tile_ranks(unsigned kept, uint32_t* wave_total, uint32_t rank[kRounds], uint32_t* start, uint32_t* all) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const unsigned long long lower = (1ull << lane) - 1ull;
    uint32_t held = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const unsigned long long round_kept = __ballot((kept >> r) & 1u);
        rank[r] = held + (uint32_t)__popcll(round_kept & lower);
        held += (uint32_t)__popcll(round_kept);
    }
    if (lane == 0) wave_total[wave] = held;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        if (v < wave) before += wave_total[v];
        sum += wave_total[v];
    }
    *start = before;
    *all = sum;
}

}  // namespace tilescan
}  // namespace snerf
