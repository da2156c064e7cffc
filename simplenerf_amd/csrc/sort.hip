// Q4: the sorts and the mask selection of the QA stage -- a stable least-significant-digit radix sort of uint32 keys (fp32 values
// through the order-preserving map of sort_plan.h, int32 keys with the permutation of the sort) and an order-preserving compaction of
// two fp32 arrays under one byte mask.  What the median, the tie-averaged ranks (metrics.hip) and the inverted index of the visibility
// mask (visibility_mask.hip) consume.
//
// A pass over one 8-bit digit is count -> scan -> scatter.  A tile (sort_plan.h: 2048 consecutive positions, one workgroup) is walked
// in index order: wave, then round, then lane.  In a round the lanes that hold the same digit find each other with eight ballots; a
// lane's rank among the tile's keys of its digit is the number of lower peer lanes plus what the wave counted for that digit in its
// earlier rounds (a [wave][digit] table in LDS), plus -- after a walk over the waves -- what the lower waves counted.  The counters
// of all tiles, digit-major, are scanned exclusively; a key's destination is its (digit, tile) offset plus its rank (the scatter puts
// the tile in that order in LDS first, so that a digit's keys leave as one run).  Equal digits therefore keep their input order, and nothing depends on which workgroup or wave runs first: there is no atomic in this file, so
// the same input gives the same bits on every call.  The compaction is the same three steps on one flag per position.
//
// Bound: memory.  A keys-and-order pass reads the keys twice and the indices once and writes both (20 bytes per key, 12 in the first
// pass, which takes a key's index from its position); a values pass moves 12 bytes per key.
#include "snerf_common.h"
#include "sort_plan.h"
#include "wave.h"

namespace {

using namespace snerf::sortplan;

// One pass.  keys_in is read as it is by every pass but the first of an fp32 sort (map_in), keys_out written as it is by every pass
// but the last of one (map_out).  payload_in NULL: a key's payload is its position (the first pass); payload_out32 / payload_out64
// both NULL: keys only.
struct Pass {
    const uint32_t* keys_in;
    uint32_t* keys_out;
    const uint32_t* payload_in;
    uint32_t* payload_out32;
    long long* payload_out64;
    uint32_t* counters;      // (kDigits, tiles): written by the count kernel, scanned, read by the scatter kernel
    long long count;
    long long tiles;
    int pass;
    int map_in;
    int map_out;
};

// Walks the calling wave's part of `tile`: key[r] is the (mapped) key of round r, rank[r] how many keys with its digit the wave holds
// before it, wave_count[wave][d] the wave's number of keys with digit d on return.  A lane whose position is past `count` takes part
// in no ballot and adds nothing.  wave_count must be zero on entry.
__device__ __forceinline__ void walk_tile(const Pass& p, long long tile, uint32_t (*wave_count)[kDigits], uint32_t key[kRounds],
                                          uint32_t rank[kRounds]) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const unsigned long long lower = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const long long i = tile_position(tile, wave, r, lane);
        const bool valid = i < p.count;
        uint32_t k = valid ? p.keys_in[i] : 0u;
        if (p.map_in) k = key_of_float(k);
        const int digit = digit_of(k, p.pass);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < kDigitBits; ++b) {
            const bool set = (digit >> b) & 1;
            const unsigned long long with_bit = __ballot(valid && set);
            peers &= set ? with_bit : ~with_bit;
        }
        const unsigned long long before = peers & lower;
        uint32_t seen = 0;
        if (valid) seen = wave_count[wave][digit];
        snerf::wave_lds_sync();
        if (valid && before == 0ull) wave_count[wave][digit] = seen + (uint32_t)__popcll(peers);   // (the lowest peer writes for all)
        snerf::wave_lds_sync();
        key[r] = k;
        rank[r] = seen + (uint32_t)__popcll(before);
    }
}

__device__ __forceinline__ void clear_wave_counts(uint32_t (*wave_count)[kDigits]) {
    for (int j = threadIdx.x; j < kWaves * kDigits; j += kBlock) (&wave_count[0][0])[j] = 0u;
    __syncthreads();
}

// grid (tiles): counters[digit][tile] = the tile's number of keys with that digit (thread t folds digit t over the waves)
__global__ void __launch_bounds__(kBlock) count_kernel(Pass p) {
    __shared__ uint32_t wave_count[kWaves][kDigits];
    const long long tile = blockIdx.x;
    uint32_t key[kRounds], rank[kRounds];
    clear_wave_counts(wave_count);
    walk_tile(p, tile, wave_count, key, rank);
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) total += wave_count[v][threadIdx.x];
    p.counters[counter_index((int)threadIdx.x, tile, p.tiles)] = total;
}

// ------------------------------------------------------------------------------------------------ workgroup scan
__device__ __forceinline__ uint32_t wave_inclusive_add_u32(uint32_t v) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t n = __shfl_up(v, off, kWave);
        if (lane >= off) v += n;
    }
    return v;
}

// Exclusive scan of `v` over the workgroup in thread order; `total` (optional) receives the workgroup's sum.  `lds` holds kWaves values.
__device__ __forceinline__ uint32_t block_exclusive_add(uint32_t v, uint32_t* lds, uint32_t* total) {
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
    if (total) *total = all;
    return before + inclusive - v;
}

// ------------------------------------------------------------------------------------------------ scatter
// grid (tiles): after the scan counters[digit][tile] is where the tile's first key with that digit goes.  Thread t scans the tile's
// own digit totals (where digit t begins in the SORTED tile) and turns column t of wave_count into the waves' starts inside it; every
// key, with its payload, is put at its sorted position in LDS; then thread t writes the sorted positions t, t + 256, ...: the keys of one
// digit leave as one contiguous run, neighbouring threads to neighbouring addresses (against one 4-byte store per key at an address
// of its own this halves the kernel's time on the 2.3 M splat keys).
__global__ void __launch_bounds__(kBlock) scatter_kernel(Pass p) {
    __shared__ uint32_t wave_count[kWaves][kDigits];
    __shared__ uint32_t shift_of_digit[kDigits];     // destination of a key = its sorted position in the tile + this, of its digit
    __shared__ uint32_t tile_keys[kTile], tile_payload[kTile];
    __shared__ uint32_t lds[kWaves];
    const long long tile = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const bool with_payload = p.payload_out32 || p.payload_out64;
    uint32_t key[kRounds], rank[kRounds];
    clear_wave_counts(wave_count);
    walk_tile(p, tile, wave_count, key, rank);
    __syncthreads();
    uint32_t held[kWaves], total = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        held[v] = wave_count[v][threadIdx.x];
        total += held[v];
    }
    uint32_t start = block_exclusive_add(total, lds, nullptr);     // where digit t begins in the sorted tile
    shift_of_digit[threadIdx.x] = p.counters[counter_index((int)threadIdx.x, tile, p.tiles)] - start;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        wave_count[v][threadIdx.x] = start;
        start += held[v];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const long long i = tile_position(tile, wave, r, lane);
        if (i >= p.count) continue;
        const uint32_t at = wave_count[wave][digit_of(key[r], p.pass)] + rank[r];
        if (at >= (uint32_t)kTile) continue;   // (cannot happen: ranks of this tile)
        tile_keys[at] = key[r];
        if (with_payload) tile_payload[at] = p.payload_in ? p.payload_in[i] : (uint32_t)i;
    }
    __syncthreads();
    const long long remaining = p.count - tile * kTile;
    const int valid = remaining < kTile ? (int)remaining : kTile;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int at = r * kBlock + (int)threadIdx.x;
        if (at >= valid) continue;
        const uint32_t k = tile_keys[at];
        const long long to = (long long)(uint32_t)((uint32_t)at + shift_of_digit[digit_of(k, p.pass)]);
        if (to >= p.count) continue;   // (cannot happen with counters of this pass; never write outside the buffers)
        p.keys_out[to] = p.map_out ? float_of_key(k) : k;
        if (p.payload_out64) p.payload_out64[to] = (long long)tile_payload[at];
        else if (p.payload_out32) p.payload_out32[to] = tile_payload[at];
    }
}

// ------------------------------------------------------------------------------------------------ the counter scan
// grid (chunks of `values`): sums[chunk] = sum of the chunk's values
__global__ void __launch_bounds__(kBlock) chunk_sums_kernel(const uint32_t* __restrict__ values, long long n, uint32_t* __restrict__ sums) {
    __shared__ uint32_t lds[kWaves];
    const long long first = (long long)blockIdx.x * kScanChunk + (long long)threadIdx.x * kScanItems;
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) mine += first + j < n ? values[first + j] : 0u;
    uint32_t total;
    block_exclusive_add(mine, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// grid (chunks of `values`): every chunk scanned exclusively in place, started at offsets[chunk] (NULL: at 0)
__global__ void __launch_bounds__(kBlock) scan_chunks_kernel(uint32_t* __restrict__ values, long long n, const uint32_t* __restrict__ offsets) {
    __shared__ uint32_t lds[kWaves];
    const long long first = (long long)blockIdx.x * kScanChunk + (long long)threadIdx.x * kScanItems;
    uint32_t item[kScanItems], mine = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        item[j] = first + j < n ? values[first + j] : 0u;
        mine += item[j];
    }
    uint32_t running = block_exclusive_add(mine, lds, nullptr) + (offsets ? offsets[blockIdx.x] : 0u);
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        if (first + j < n) values[first + j] = running;
        running += item[j];
    }
}

inline unsigned chunks(long long n) { return (unsigned)((n + kScanChunk - 1) / kScanChunk); }

// Enqueues the exclusive scan of level 0 of `plan` (sort_plan.h), in place.
void enqueue_scan(const ScanPlan& plan, char* workspace, hipStream_t stream) {
    auto level = [&](int l) { return (uint32_t*)(workspace + plan.offset[l]); };
    const int top = plan.levels - 1;
    for (int l = 0; l < top; ++l)
        hipLaunchKernelGGL(chunk_sums_kernel, dim3(chunks(plan.size[l])), dim3(kBlock), 0, stream, (const uint32_t*)level(l), plan.size[l],
                           level(l + 1));
    hipLaunchKernelGGL(scan_chunks_kernel, dim3(1), dim3(kBlock), 0, stream, level(top), plan.size[top], (const uint32_t*)nullptr);
    for (int l = top - 1; l >= 0; --l)
        hipLaunchKernelGGL(scan_chunks_kernel, dim3(chunks(plan.size[l])), dim3(kBlock), 0, stream, level(l), plan.size[l],
                           (const uint32_t*)level(l + 1));
}

// All passes of one sort.  keys: the caller's input; out_keys: the caller's output (uint32 or, with `floats`, fp32 bit patterns);
// order: the caller's int64 permutation or NULL.  An intermediate pass on the caller's side keeps its uint32 indices in the first
// half of `order`, which only the last pass -- reading the workspace's side -- overwrites with the int64 values.
void enqueue_sort(const SortPlan& plan, const uint32_t* keys, uint32_t* out_keys, long long* order, bool floats, char* workspace,
                  hipStream_t stream) {
    uint32_t* side_keys[2] = {out_keys, (uint32_t*)(workspace + plan.keys_offset)};
    uint32_t* side_payload[2] = {(uint32_t*)order, (uint32_t*)(workspace + plan.payload_offset)};
    Pass p;
    p.keys_in = keys;
    p.payload_in = nullptr;
    p.counters = (uint32_t*)(workspace + plan.scan.offset[0]);
    p.count = plan.count;
    p.tiles = plan.tiles;
    for (int pass = 0; pass < plan.passes; ++pass) {
        const int side = side_written(pass, plan.passes);
        const bool last = pass == plan.passes - 1;
        p.pass = pass;
        p.map_in = floats && pass == 0;
        p.map_out = floats && last;
        p.keys_out = side_keys[side];
        p.payload_out32 = order && !last ? side_payload[side] : nullptr;
        p.payload_out64 = order && last ? order : nullptr;
        hipLaunchKernelGGL(count_kernel, dim3((unsigned)plan.tiles), dim3(kBlock), 0, stream, p);
        enqueue_scan(plan.scan, workspace, stream);
        hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)plan.tiles), dim3(kBlock), 0, stream, p);
        p.keys_in = p.keys_out;
        p.payload_in = p.payload_out32;
    }
}

// ------------------------------------------------------------------------------------------------ compaction
// Bit r of the result: the calling lane's position of round r is inside `count` and its mask byte is not zero.
__device__ __forceinline__ unsigned kept_rounds(const unsigned char* __restrict__ mask, long long count, long long tile) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned kept = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const long long i = tile_position(tile, wave, r, lane);
        if (i < count && mask[i] != 0) kept |= 1u << r;
    }
    return kept;
}

// grid (tiles): counters[tile] = the tile's number of kept positions
__global__ void __launch_bounds__(kBlock) compact_count_kernel(const unsigned char* __restrict__ mask, long long count,
                                                               uint32_t* __restrict__ counters) {
    __shared__ uint32_t lds[kWaves];
    const unsigned kept = kept_rounds(mask, count, blockIdx.x);
    uint32_t total;
    block_exclusive_add((uint32_t)__popc(kept), lds, &total);
    if (threadIdx.x == 0) counters[blockIdx.x] = total;
}

// grid (tiles): counters scanned.  A kept position goes to the tile's start + what the lower waves keep + what the wave keeps in its
// earlier rounds + the number of lower kept lanes of its round: ascending positions, no atomics.  The last tile writes the count.
__global__ void __launch_bounds__(kBlock) compact_scatter_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const unsigned char* __restrict__ mask, long long count,
                                                                 const uint32_t* __restrict__ counters, float* __restrict__ a_kept,
                                                                 float* __restrict__ b_kept, long long* __restrict__ kept_count) {
    __shared__ uint32_t wave_total[kWaves];
    const long long tile = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const unsigned long long lower = (1ull << lane) - 1ull;
    const unsigned kept = kept_rounds(mask, count, tile);
    uint32_t rank[kRounds], held = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const unsigned long long round_kept = __ballot((kept >> r) & 1u);
        rank[r] = held + (uint32_t)__popcll(round_kept & lower);
        held += (uint32_t)__popcll(round_kept);
    }
    if (lane == 0) wave_total[wave] = held;
    __syncthreads();
    uint32_t start = counters[tile], all = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        if (v < wave) start += wave_total[v];
        all += wave_total[v];
    }
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        if (!((kept >> r) & 1u)) continue;
        const long long i = tile_position(tile, wave, r, lane), to = (long long)start + rank[r];
        if (to >= count) continue;   // (cannot happen with counters of this mask; never write outside the buffers)
        a_kept[to] = a[i];
        b_kept[to] = b[i];
    }
    if (tile == (long long)gridDim.x - 1 && threadIdx.x == 0) kept_count[0] = (long long)counters[tile] + all;
}

__global__ void zero_count_kernel(long long* kept_count) { kept_count[0] = 0; }

}  // namespace

extern "C" long long snerf_sort_workspace_bytes(long long count, int key_bits) {
    SortPlan plan;
    return plan_sort(count, key_bits, plan) ? plan.bytes : 0;
}

extern "C" int snerf_sort_f32(const float* values, long long count, float* sorted, void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(count >= 0 && count <= kMaxCount, "sort_f32: count %lld outside 0 .. 2^31 - 1", count);
    if (count == 0) return SNERF_OK;
    SNERF_REQUIRE(values, "sort_f32: values is NULL");
    SNERF_REQUIRE(sorted, "sort_f32: sorted is NULL");
    SNERF_REQUIRE(workspace, "sort_f32: workspace is NULL");
    SNERF_REQUIRE((const void*)values != (const void*)sorted, "sort_f32: sorted must not be values (the input is never written)");
    SortPlan plan;
    SNERF_REQUIRE(plan_sort(count, 32, plan), "sort_f32: count %lld cannot be planned", count);
    enqueue_sort(plan, (const uint32_t*)values, (uint32_t*)sorted, nullptr, true, (char*)workspace, (hipStream_t)stream);
    return snerf::check_launch("sort_f32");
}

extern "C" int snerf_sort_keys_with_order(const int* keys, long long count, int key_bits, int* sorted_keys, long long* order,
                                          void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(key_bits >= 1 && key_bits <= 32, "sort_keys_with_order: key_bits %d outside 1 .. 32", key_bits);
    SNERF_REQUIRE(count >= 0 && count <= kMaxCount, "sort_keys_with_order: count %lld outside 0 .. 2^31 - 1", count);
    if (count == 0) return SNERF_OK;
    SNERF_REQUIRE(keys, "sort_keys_with_order: keys is NULL");
    SNERF_REQUIRE(sorted_keys, "sort_keys_with_order: sorted_keys is NULL");
    SNERF_REQUIRE(order, "sort_keys_with_order: order is NULL");
    SNERF_REQUIRE(workspace, "sort_keys_with_order: workspace is NULL");
    SNERF_REQUIRE(keys != sorted_keys, "sort_keys_with_order: sorted_keys must not be keys (the input is never written)");
    SortPlan plan;
    SNERF_REQUIRE(plan_sort(count, key_bits, plan), "sort_keys_with_order: count %lld cannot be planned", count);
    enqueue_sort(plan, (const uint32_t*)keys, (uint32_t*)sorted_keys, order, false, (char*)workspace, (hipStream_t)stream);
    return snerf::check_launch("sort_keys_with_order");
}

extern "C" long long snerf_compact_workspace_bytes(long long count) {
    CompactPlan plan;
    return plan_compact(count, plan) ? plan.bytes : 0;
}

extern "C" int snerf_compact_f32_pair(const float* a, const float* b, const unsigned char* mask, long long count, float* a_kept,
                                      float* b_kept, long long* kept, void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(count >= 0 && count <= kMaxCount, "compact_f32_pair: count %lld outside 0 .. 2^31 - 1", count);
    SNERF_REQUIRE(kept, "compact_f32_pair: kept is NULL");
    if (count == 0) {
        hipLaunchKernelGGL(zero_count_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, kept);
        return snerf::check_launch("compact_f32_pair");
    }
    SNERF_REQUIRE(a && b, "compact_f32_pair: a or b is NULL");
    SNERF_REQUIRE(mask, "compact_f32_pair: mask is NULL");
    SNERF_REQUIRE(a_kept && b_kept, "compact_f32_pair: a_kept or b_kept is NULL");
    SNERF_REQUIRE(workspace, "compact_f32_pair: workspace is NULL");
    CompactPlan plan;
    SNERF_REQUIRE(plan_compact(count, plan), "compact_f32_pair: count %lld cannot be planned", count);
    uint32_t* counters = (uint32_t*)((char*)workspace + plan.scan.offset[0]);
    hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)plan.tiles), dim3(kBlock), 0, (hipStream_t)stream, mask, count, counters);
    enqueue_scan(plan.scan, (char*)workspace, (hipStream_t)stream);
    hipLaunchKernelGGL(compact_scatter_kernel, dim3((unsigned)plan.tiles), dim3(kBlock), 0, (hipStream_t)stream, a, b, mask, count,
                       (const uint32_t*)counters, a_kept, b_kept, kept);
    return snerf::check_launch("compact_f32_pair");
}
