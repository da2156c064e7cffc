// simplenerf_amd/csrc/sort_plan.h on the host (no GPU; built with AddressSanitizer + UBSan by tests/test_sort_host.py): the fp32 key
// map's order and inverse, the tiles' cover of [0, count), the counter layout, the workspace regions and the ping-pong of the passes.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../simplenerf_amd/csrc/sort_plan.h"

using namespace snerf::sortplan;

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) { std::printf("check failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; }   \
    } while (0)

static uint32_t bits_of(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}
static float float_of(uint32_t b) {
    float v;
    std::memcpy(&v, &b, 4);
    return v;
}

static int check_key_map() {
    const float inf = std::numeric_limits<float>::infinity();
    const float denorm = std::numeric_limits<float>::denorm_min();
    // strictly ascending by the rule of the header: -0 before +0
    const std::vector<float> ladder = {-inf, -3.5f, -1.f, -1e-30f, -8 * denorm, -denorm, -0.f, 0.f, denorm, 8 * denorm, 1e-30f, 1.f, 3.5f, inf};
    for (size_t i = 0; i + 1 < ladder.size(); ++i) CHECK(key_of_float(bits_of(ladder[i])) < key_of_float(bits_of(ladder[i + 1])));
    CHECK(key_of_float(bits_of(-0.f)) + 1 == key_of_float(bits_of(0.f)));
    for (float v : ladder) CHECK(float_of_key(key_of_float(bits_of(v))) == bits_of(v));   // the inverse restores the bits
    // every NaN after +inf, returned as the canonical one
    for (uint32_t nan : {0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0xFF800001u, 0x7FFFFFFFu, 0xFFFFFFFFu, 0x7FC12345u}) {
        CHECK(std::isnan(float_of(nan)));
        CHECK(key_of_float(nan) > key_of_float(bits_of(inf)));
        CHECK(key_of_float(nan) == key_of_float(kCanonicalNan));
        CHECK(float_of_key(key_of_float(nan)) == kCanonicalNan);
    }
    // 10^5 random pairs of bit patterns: the keys order as the values do
    std::mt19937 rng(20240607u);
    int compared = 0;
    while (compared < 100000) {
        const uint32_t a = rng(), b = rng();
        const float x = float_of(a), y = float_of(b);
        if (std::isnan(x) || std::isnan(y)) continue;
        ++compared;
        const uint32_t ka = key_of_float(a), kb = key_of_float(b);
        if (x < y) CHECK(ka < kb);
        if (x > y) CHECK(ka > kb);
        if (x == y && a == b) CHECK(ka == kb);
        CHECK(float_of_key(ka) == a && float_of_key(kb) == b);
    }
    // and pairs that are close: neighbouring patterns around a random value, across zero included
    for (int i = 0; i < 100000; ++i) {
        const uint32_t a = rng() & 0xFF800FFFu, b = a + 1;   // (small mantissas: b is the next pattern away from zero)
        const float x = float_of(a), y = float_of(b);
        if (std::isnan(x) || std::isnan(y) || std::isinf(y)) continue;
        if (x < y) CHECK(key_of_float(a) < key_of_float(b));
        if (x > y) CHECK(key_of_float(a) > key_of_float(b));
    }
    return 0;
}

static int check_scan(const ScanPlan& scan, long long counters, long long first_byte, long long bytes) {
    CHECK(scan.levels >= 1 && scan.levels <= kMaxScanLevels);
    CHECK(scan.size[0] == counters && scan.offset[0] == first_byte);
    for (int l = 0; l < scan.levels; ++l) {
        CHECK(scan.offset[l] % kAlign == 0 && scan.offset[l] + scan.size[l] * 4 <= bytes);
        if (l + 1 < scan.levels) {
            CHECK(scan.size[l] > kScanChunk);                                          // a level above exists only where needed
            CHECK(scan.size[l + 1] == (scan.size[l] + kScanChunk - 1) / kScanChunk);   // one sum per chunk
            CHECK(scan.offset[l + 1] >= scan.offset[l] + scan.size[l] * 4);            // disjoint, ascending
        }
    }
    CHECK(scan.size[scan.levels - 1] <= kScanChunk);   // the top level is one workgroup's step
    return 0;
}

static int check_count(long long count, bool walk) {
    const long long num_tiles = tiles(count);
    CHECK(num_tiles >= 1 && (num_tiles - 1) * kTile < count && count <= num_tiles * kTile);
    if (walk) {
        // the tiles cover [0, count) exactly once, and (tile, wave, round, lane) ascending is position ascending
        std::vector<unsigned char> seen(count, 0);
        long long previous = -1;
        for (long long tile = 0; tile < num_tiles; ++tile)
            for (int wave = 0; wave < kWaves; ++wave)
                for (int round = 0; round < kRounds; ++round)
                    for (int lane = 0; lane < kWave; ++lane) {
                        const long long i = tile_position(tile, wave, round, lane);
                        CHECK(i == previous + 1);
                        previous = i;
                        if (i < count) seen[i] += 1;
                    }
        CHECK(previous + 1 == num_tiles * kTile);
        for (long long i = 0; i < count; ++i) CHECK(seen[i] == 1);
        // the counter index is a bijection onto 256 x tiles, digit-major
        std::vector<unsigned char> hit(kDigits * num_tiles, 0);
        for (int digit = 0; digit < kDigits; ++digit)
            for (long long tile = 0; tile < num_tiles; ++tile) {
                const long long c = counter_index(digit, tile, num_tiles);
                CHECK(c >= 0 && c < kDigits * num_tiles);
                hit[c] += 1;
                if (tile + 1 < num_tiles) CHECK(counter_index(digit, tile + 1, num_tiles) == c + 1);
            }
        for (unsigned char h : hit) CHECK(h == 1);
    }
    for (int key_bits : {1, 8, 9, 16, 17, 22, 24, 25, 32}) {
        SortPlan plan;
        CHECK(plan_sort(count, key_bits, plan));
        CHECK(plan.count == count && plan.tiles == num_tiles && plan.passes == (key_bits + 7) / 8);
        CHECK(plan.keys_offset % kAlign == 0 && plan.payload_offset % kAlign == 0);
        CHECK(plan.keys_offset + count * 4 <= plan.payload_offset);
        CHECK(plan.payload_offset + count * 4 <= plan.scan.offset[0]);
        if (check_scan(plan.scan, kDigits * num_tiles, plan.scan.offset[0], plan.bytes)) return 1;
    }
    CompactPlan compact;
    CHECK(plan_compact(count, compact) && compact.tiles == num_tiles);
    if (check_scan(compact.scan, num_tiles, 0, compact.bytes)) return 1;
    return 0;
}

int main() {
    static_assert(kTile == kBlock * kRounds && kWaves * kWave == kBlock && kDigits == kBlock, "one thread per digit, kRounds keys per thread");
    if (check_key_map()) return 1;
    const long long counts[] = {1, 2, 63, 64, 65, kTile - 1, kTile, kTile + 1, 3 * kTile + 17, 762048, 2292000};
    for (long long count : counts)
        if (check_count(count, true)) return 1;
    // the counts at which the counter scan gains a level (2048 counters a step: above 16 384 keys two levels, above 2^25 three), and
    // the largest: the plans only
    for (long long count : {16384LL, 16385LL, 33554432LL, 33554433LL, 40000000LL, kMaxCount}) {
        if (check_count(count, false)) return 1;
    }
    {
        SortPlan plan;
        CHECK(plan_sort(kMaxCount, 32, plan) && plan.scan.levels == 3);
        CHECK(plan_sort(16384, 32, plan) && plan.scan.levels == 1);
        CHECK(plan_sort(16385, 32, plan) && plan.scan.levels == 2);
        CHECK(plan_sort(33554432, 32, plan) && plan.scan.levels == 2);
        CHECK(plan_sort(33554433, 32, plan) && plan.scan.levels == 3);
        CHECK(plan_sort(2292000, 22, plan) && plan.scan.levels == 2 && plan.passes == 3);
        CHECK(plan_sort(kTile, 8, plan) && plan.scan.levels == 1 && plan.passes == 1);
        CHECK(!plan_sort(0, 32, plan) && !plan_sort(-1, 32, plan) && !plan_sort(kMaxCount + 1, 32, plan));
        CHECK(!plan_sort(100, 0, plan) && !plan_sort(100, 33, plan));
        CompactPlan compact;
        CHECK(!plan_compact(0, compact) && !plan_compact(kMaxCount + 1, compact));
    }
    // workspace sizes never shrink as the count grows
    long long last_sort = 0, last_compact = 0;
    for (long long count = 1; count < 70000; count += 97) {
        SortPlan plan;
        CompactPlan compact;
        CHECK(plan_sort(count, 32, plan) && plan_compact(count, compact));
        CHECK(plan.bytes >= last_sort && compact.bytes >= last_compact);
        last_sort = plan.bytes;
        last_compact = compact.bytes;
    }
    // the ping-pong: the last pass writes the caller's output, consecutive passes alternate, so a pass never reads what it writes
    for (int num_passes = 1; num_passes <= 4; ++num_passes) {
        CHECK(side_written(num_passes - 1, num_passes) == 0);
        for (int pass = 0; pass + 1 < num_passes; ++pass) CHECK(side_written(pass, num_passes) != side_written(pass + 1, num_passes));
    }
    // digits
    CHECK(digit_of(0x12345678u, 0) == 0x78 && digit_of(0x12345678u, 1) == 0x56 && digit_of(0x12345678u, 3) == 0x12);
    CHECK(passes(1) == 1 && passes(8) == 1 && passes(9) == 2 && passes(22) == 3 && passes(32) == 4);
    std::printf("sort_plan_test: OK\n");
    return 0;
}
