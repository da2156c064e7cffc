// Key map, tiling, counter layout and workspace plan of the radix sort and the mask compaction (sort.hip), in a header of its own so
// that a plain C++ program can walk them on the host (tests/native/sort_plan_test.cpp: the map's order, the tiles' cover, the counter
// bijection and the workspace regions, under AddressSanitizer).  No HIP types.
//
// The sort is least-significant-digit first on 8-bit digits.  A pass cuts the positions into TILES of kTile consecutive keys, one
// workgroup each; within a tile wave `v` owns the kWaveKeys consecutive positions from v * kWaveKeys and walks them in kRounds rounds
// of 64, so the order (wave, round, lane) IS the index order -- what makes the ranks of equal digits stable.  A pass counts every
// tile's digits into counters laid out digit-major (all tiles of digit 0, then of digit 1, ...): their exclusive scan is, for every
// (digit, tile), the output position of the tile's first key with that digit.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SNERF_SORT_FN __host__ __device__ __forceinline__
#else
#define SNERF_SORT_FN inline
#endif

namespace snerf {
namespace sortplan {

constexpr int kDigitBits = 8;
constexpr int kDigits = 1 << kDigitBits;
constexpr int kBlock = 256;                     // threads of every kernel of sort.hip
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kRounds = 8;                      // keys per thread
constexpr int kWaveKeys = kRounds * kWave;      // consecutive positions one wave owns
constexpr int kTile = kWaves * kWaveKeys;       // consecutive positions one workgroup owns (2048)
constexpr int kScanItems = 8;                   // counters per thread of the scan kernels
constexpr int kScanChunk = kBlock * kScanItems; // counters one workgroup scans in one step (2048)
constexpr int kMaxScanLevels = 3;               // 256 * 2^20 counters -> 2^17 chunk sums -> 64: the largest count needs three
constexpr long long kMaxCount = 2147483647LL;   // counts stay below 2^31: positions and counter sums fit uint32
constexpr long long kAlign = 256;               // every workspace region starts on a multiple of this

// ------------------------------------------------------------------------------------------------ fp32 keys
constexpr uint32_t kCanonicalNan = 0x7FC00000u;

// Order-preserving map of an fp32 bit pattern to uint32: all bits of a negative value are flipped, only the sign bit otherwise, so
// -inf < ... < -0 < +0 < ... < +inf compare as unsigned integers.  Every NaN, whatever its sign and payload, takes the key of the
// canonical quiet NaN, above +inf.
SNERF_SORT_FN uint32_t key_of_float(uint32_t bits) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) bits = kCanonicalNan;
    return (bits & 0x80000000u) ? ~bits : (bits ^ 0x80000000u);
}

SNERF_SORT_FN uint32_t float_of_key(uint32_t key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

// ------------------------------------------------------------------------------------------------ tiles and counters
SNERF_SORT_FN int passes(int key_bits) { return (key_bits + kDigitBits - 1) / kDigitBits; }
SNERF_SORT_FN long long tiles(long long count) { return (count + kTile - 1) / kTile; }
SNERF_SORT_FN int digit_of(uint32_t key, int pass) { return (int)((key >> (pass * kDigitBits)) & (uint32_t)(kDigits - 1)); }

// The position a lane reads in a round (it takes part when the position is below `count`).
SNERF_SORT_FN long long tile_position(long long tile, int wave, int round, int lane) {
    return tile * kTile + (long long)wave * kWaveKeys + (long long)round * kWave + lane;
}

SNERF_SORT_FN long long counter_index(int digit, long long tile, long long num_tiles) { return (long long)digit * num_tiles + tile; }

// Which buffer pass `pass` of `num_passes` writes: 0 = the caller's output, 1 = the workspace.  The last pass writes the caller's
// output, the one before it the workspace, and so on; pass 0 reads the caller's input, which is never written.
SNERF_SORT_FN int side_written(int pass, int num_passes) { return (num_passes - 1 - pass) & 1; }

// ------------------------------------------------------------------------------------------------ the counter scan
// An exclusive scan of n uint32 counters in place: level 0 is the counters, level l + 1 holds one sum per kScanChunk values of level l,
// until a level fits one chunk.  That level is scanned by one workgroup; going back down, every chunk is scanned and takes the
// scanned sum of the level above as its offset.
struct ScanPlan {
    int levels;                          // 1 .. kMaxScanLevels
    long long size[kMaxScanLevels];      // values of level l
    long long offset[kMaxScanLevels];    // byte offset of level l in the workspace (level 0: the counters themselves)
};

SNERF_SORT_FN long long align_up(long long bytes) { return (bytes + kAlign - 1) / kAlign * kAlign; }

// Fills `plan` for n >= 1 counters placed at byte `at`; -> the first byte after the last level.  0 levels (and `at` back) when n
// needs more than kMaxScanLevels levels, which no count below 2^31 does.
SNERF_SORT_FN long long plan_scan(long long n, long long at, ScanPlan& plan) {
    plan.levels = 0;
    long long size = n;
    for (int l = 0; l < kMaxScanLevels; ++l) {
        plan.size[l] = size;
        plan.offset[l] = at;
        at += align_up(size * 4);
        plan.levels = l + 1;
        if (size <= kScanChunk) return at;
        size = (size + kScanChunk - 1) / kScanChunk;
    }
    plan.levels = 0;
    return plan.offset[0];
}

// ------------------------------------------------------------------------------------------------ workspaces
struct SortPlan {
    long long count;
    int passes;
    long long tiles;
    long long keys_offset;       // count uint32: the keys' second buffer
    long long payload_offset;    // count uint32: the source indices' second buffer (snerf_sort_keys_with_order)
    ScanPlan scan;               // 256 * tiles counters and the levels above them
    long long bytes;
};

// false: count outside 1 .. 2^31 - 1 or key_bits outside 1 .. 32
SNERF_SORT_FN bool plan_sort(long long count, int key_bits, SortPlan& plan) {
    if (count < 1 || count > kMaxCount || key_bits < 1 || key_bits > 32) return false;
    plan.count = count;
    plan.passes = passes(key_bits);
    plan.tiles = tiles(count);
    plan.keys_offset = 0;
    plan.payload_offset = align_up(count * 4);
    plan.bytes = plan_scan((long long)kDigits * plan.tiles, plan.payload_offset + align_up(count * 4), plan.scan);
    return plan.scan.levels > 0;
}

struct CompactPlan {
    long long count;
    long long tiles;
    ScanPlan scan;               // one counter per tile (its kept elements) and the levels above them
    long long bytes;
};

SNERF_SORT_FN bool plan_compact(long long count, CompactPlan& plan) {
    if (count < 1 || count > kMaxCount) return false;
    plan.count = count;
    plan.tiles = tiles(count);
    plan.bytes = plan_scan(plan.tiles, 0, plan.scan);
    return plan.scan.levels > 0;
}

}  // namespace sortplan
}  // namespace snerf
