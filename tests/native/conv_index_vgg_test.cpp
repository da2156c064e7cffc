// Walks the VGG-16 part of simplenerf_amd/csrc/conv_index.h on the host (built with -fsanitize=address,undefined by
// tests/test_lpips_vgg_host.py): for every image extent given on the command line ("h w" pairs) it
//   * checks every convolution's and every tap's extents against the closed forms (a 3 x 3 stride-1 pad-1 convolution keeps the
//     extent, the 2 x 2 stride-2 pool halves it rounding down: tap t has floor(in / 2^t)),
//   * enumerates every (output pixel, k) of every layer's implicit GEMM and compares k's tap and the source coordinate / padding
//     predicate with a direct triple loop over (tap row, tap column, channel), touching the source tensor at every in-range
//     coordinate (a wrong index is an out-of-bounds access the sanitizer reports) and counting that every source element is hit;
//     where c_in is a multiple of the slab it also checks what the kernel relies on there: the 32 values of k of a slab share the
//     tap of the slab's first k, and their channels are consecutive,
//   * checks that every pool window lies inside its source and that the windows cover it up to the floor-mode remainder,
//   * checks the workspace plan: regions aligned, inside the total, pairwise disjoint, each large enough for every tensor the plan
//     puts there, and no convolution reading the region it writes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../simplenerf_amd/csrc/conv_index.h"

using namespace snerf::conv_index;

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            std::printf("conv_index_vgg_test: FAILED %s: ", #cond); \
            std::printf(__VA_ARGS__);                         \
            std::printf("\n");                                \
            return 1;                                         \
        }                                                     \
    } while (0)

static int closed_conv(int in) { return (int)std::floor((double)(in + 2 * 1 - 3) / 1) + 1; }
static int closed_pool(int in) { return (int)std::floor((double)(in - 2) / 2) + 1; }

static int walk_pool(int in_h, int in_w) {
    const int out_h = vgg_pool_extent(in_h), out_w = vgg_pool_extent(in_w);
    CHECK(out_h == closed_pool(in_h) && out_w == closed_pool(in_w) && out_h == in_h / 2 && out_w == in_w / 2 && out_h >= 1 && out_w >= 1,
          "pool of %d x %d", in_h, in_w);
    std::vector<unsigned char> seen((size_t)in_h * in_w, 0);
    for (int oy = 0; oy < out_h; ++oy)
        for (int ox = 0; ox < out_w; ++ox)
            for (int dy = 0; dy < kVggPoolWindow; ++dy)
                for (int dx = 0; dx < kVggPoolWindow; ++dx) {
                    const int y = vgg_pool_first(oy) + dy, x = vgg_pool_first(ox) + dx;
                    CHECK(y == 2 * oy + dy && x == 2 * ox + dx, "pool window origin of (%d, %d)", oy, ox);
                    CHECK(y >= 0 && y < in_h && x >= 0 && x < in_w, "pool window (%d, %d) + (%d, %d) leaves %d x %d", oy, ox, dy, dx, in_h, in_w);
                    CHECK(seen[(size_t)y * in_w + x] == 0, "pool windows overlap at (%d, %d)", y, x);      // stride = window
                    seen[(size_t)y * in_w + x] = 1;
                }
    // floor mode: an odd extent's last row / column is never read, everything before is, once
    for (int y = 0; y < in_h; ++y)
        for (int x = 0; x < in_w; ++x) CHECK(seen[(size_t)y * in_w + x] == (y < 2 * out_h && x < 2 * out_w ? 1 : 0), "pool coverage at (%d, %d)", y, x);
    CHECK(in_h - 2 * out_h == in_h % 2 && in_w - 2 * out_w == in_w % 2, "pool remainder");
    return 0;
}

// the geometry is a template argument, as in the kernel: the divisions of k_tap are by constants
template <int L>
static int walk_conv(int in_h, int in_w, long long* visited) {
    constexpr ConvGeom g = kVggGeom[L];
    static_assert(g.kernel == 3 && g.stride == 1 && g.pad == 1 && g.c_out % 64 == 0, "VGG-16's convolutions");
    constexpr bool slab_in_tap = g.c_in % kSlab == 0;
    const int out_h = conv_extent(in_h, g), out_w = conv_extent(in_w, g);
    CHECK(out_h == closed_conv(in_h) && out_w == closed_conv(in_w) && out_h == in_h && out_w == in_w, "conv extents of layer %d", L);
    CHECK(k_count(g) == 9 * g.c_in && k_padded(g) % kSlab == 0 && k_padded(g) >= k_count(g) && k_padded(g) - k_count(g) < kSlab, "k padding");
    CHECK(!slab_in_tap || k_padded(g) == k_count(g), "whole slabs in layer %d", L);
    std::vector<unsigned char> source((size_t)in_h * in_w * g.c_in, 0);     // touched through the header's indices
    for (int oy = 0; oy < out_h; ++oy)
        for (int ox = 0; ox < out_w; ++ox) {
            int k = 0;
            for (int ky = 0; ky < g.kernel; ++ky)
                for (int kx = 0; kx < g.kernel; ++kx) {
                    const int iy = source_origin(g, oy) + ky, ix = source_origin(g, ox) + kx;
                    CHECK(iy == oy - 1 + ky && ix == ox - 1 + kx, "source of (%d, %d) tap (%d, %d)", oy, ox, ky, kx);
                    const bool inside = in_source(iy, in_h) && in_source(ix, in_w);
                    CHECK(inside == (iy >= 0 && iy < in_h && ix >= 0 && ix < in_w), "padding predicate at (%d, %d)", iy, ix);
                    unsigned char* pixel = inside ? &source[((size_t)iy * in_w + ix) * g.c_in] : nullptr;
                    for (int c = 0; c < g.c_in; ++c, ++k) {
                        const Tap t = k_tap(g, k);
                        CHECK(t.ky == ky && t.kx == kx && t.c == c && k_index(g, ky, kx, c) == k, "k %d -> (%d, %d, %d)", k, t.ky, t.kx, t.c);
                        // a slab that starts here ends inside this tap: with t.c == c for every k, its k0 + j is (ky, kx, c + j)
                        if (slab_in_tap && k % kSlab == 0) CHECK(c + kSlab <= g.c_in, "slab of k %d", k);
                        if (inside) pixel[t.c] = 1;
                    }
                }
            CHECK(k == k_count(g), "k count");
            *visited += k;
        }
    // stride 1, pad 1: every source element is under some window
    for (size_t i = 0; i < source.size(); ++i) CHECK(source[i] == 1, "source coverage at element %zu of layer %d", i, L);
    return 0;
}

template <int L>
static int walk_network(int height, int width, int& h, int& w, long long* visited) {
    if (kVggGeom[L].pool_before) {
        if (walk_pool(h, w)) return 1;
        h = vgg_pool_extent(h);
        w = vgg_pool_extent(w);
    }
    if (walk_conv<L>(h, w, visited)) return 1;
    h = conv_extent(h, kVggGeom[L]);
    w = conv_extent(w, kVggGeom[L]);
    CHECK(h == vgg_conv_output_extent(height, L) && w == vgg_conv_output_extent(width, L), "extent of convolution %d", L);
    if (kVggTapOf[L] >= 0) {
        const int tap = kVggTapOf[L];
        CHECK(kVggTapConv[tap] == L, "tap %d follows convolution %d", tap, L);
        CHECK(h == vgg_tap_extent(height, tap) && w == vgg_tap_extent(width, tap) && h == height >> tap && w == width >> tap, "extent of tap %d", tap);
        std::printf(" %d x %d", h, w);
    }
    if constexpr (L + 1 < kVggConvs) return walk_network<L + 1>(height, width, h, w, visited);
    return 0;
}

struct Region {
    const char* name;
    long long at, bytes;
};

static int check_plan(int height, int width) {
    const VggPlan p = vgg_plan(height, width);
    CHECK(p.fits, "plan of %d x %d", height, width);
    const Region regions[] = {{"input", p.input, p.input_bytes},        {"tap 0", p.tap[0], p.tap_bytes[0]},   {"tap 1", p.tap[1], p.tap_bytes[1]},
                              {"tap 2", p.tap[2], p.tap_bytes[2]},      {"tap 3", p.tap[3], p.tap_bytes[3]},   {"tap 4", p.tap[4], p.tap_bytes[4]},
                              {"ping 0", p.ping[0], p.ping_bytes[0]},   {"ping 1", p.ping[1], p.ping_bytes[1]}, {"pooled", p.pooled, p.pooled_bytes},
                              {"partials", p.partials, p.partials_bytes}};
    const int count = (int)(sizeof(regions) / sizeof(regions[0]));
    long long sum = 0;
    for (int i = 0; i < count; ++i) {
        const Region& r = regions[i];
        CHECK(r.at >= 0 && r.at % 256 == 0 && r.bytes > 0 && r.at + r.bytes <= p.total, "region %s: %lld + %lld of %lld", r.name, r.at, r.bytes, p.total);
        for (int j = 0; j < i; ++j)
            CHECK(r.at + r.bytes <= regions[j].at || regions[j].at + regions[j].bytes <= r.at, "regions %s and %s overlap", r.name, regions[j].name);
        sum += r.bytes;
    }
    CHECK(p.total >= sum && p.total - sum < 256LL * count, "total %lld against the regions' %lld", p.total, sum);
    CHECK(p.input_bytes == 4LL * 2 * height * width * 3 && p.partials_bytes == 8LL * kVggTaps * kVggMaxPartials, "input and partials");
    auto bytes_of = [&](int region) {
        return region >= 0 ? p.tap_bytes[region] : region == kVggRegionInput ? p.input_bytes : region == kVggRegionPooled ? p.pooled_bytes
                                                 : p.ping_bytes[region == kVggRegionPing0 ? 0 : 1];
    };
    int h = height, w = width;
    for (int l = 0; l < kVggConvs; ++l) {
        const ConvGeom g = kVggGeom[l];
        if (g.pool_before) {
            CHECK(l > 0 && p.target[l - 1] >= 0 && p.source[l] == kVggRegionPooled, "the pool in front of convolution %d reads a tap", l);
            h /= 2;
            w /= 2;
        } else {
            CHECK(p.source[l] == (l == 0 ? kVggRegionInput : p.target[l - 1]), "convolution %d reads what convolution %d wrote", l, l - 1);
        }
        CHECK(p.in_h[l] == h && p.in_w[l] == w && p.out_h[l] == h && p.out_w[l] == w, "extents of convolution %d in the plan", l);
        CHECK(p.source[l] != p.target[l], "convolution %d reads the region it writes", l);
        CHECK(kVggTapOf[l] >= 0 ? p.target[l] == kVggTapOf[l] : p.target[l] == kVggRegionPing0 || p.target[l] == kVggRegionPing1,
              "target of convolution %d", l);
        CHECK(bytes_of(p.source[l]) >= 4LL * 2 * h * w * g.c_in, "convolution %d's input does not fit its region", l);
        CHECK(bytes_of(p.target[l]) >= 4LL * 2 * h * w * g.c_out, "convolution %d's output does not fit its region", l);
        if (kVggTapOf[l] >= 0) CHECK(p.tap_bytes[kVggTapOf[l]] == 4LL * 2 * h * w * g.c_out, "tap %d's bytes", kVggTapOf[l]);
    }
    std::printf("plan %d x %d: %lld bytes\n", height, width, p.total);
    return 0;
}

int main(int argc, char** argv) {
    CHECK(argc >= 3 && argc % 2 == 1, "usage: conv_index_vgg_test h w [h w ...]");
    CHECK(kVggConvs == 13 && kVggTaps == 5 && kVggGeom[0].c_in == 3 && kVggGeom[12].c_out == 512, "geometry table");
    for (int l = 0; l + 1 < kVggConvs; ++l) CHECK(kVggGeom[l].c_out == kVggGeom[l + 1].c_in, "channels of layer %d", l);
    int pools = 0;
    for (int l = 0; l < kVggConvs; ++l) pools += kVggGeom[l].pool_before ? 1 : 0;
    CHECK(pools == 4 && !kVggGeom[0].pool_before, "four pools");
    CHECK(vgg_tap_extent(kVggMinExtent, 4) == 1 && vgg_tap_extent(kVggMinExtent - 1, 4) == 0 && vgg_tap_extent(kVggMinExtent - 1, 0) == 0 &&
              vgg_tap_extent(kVggMinExtent, 0) == 16, "minimum extent");
    long long visited = 0;
    for (int arg = 1; arg + 1 < argc; arg += 2) {
        const int height = std::atoi(argv[arg]), width = std::atoi(argv[arg + 1]);
        CHECK(height >= kVggMinExtent && width >= kVggMinExtent, "extent %d x %d", height, width);
        std::printf("extents %d x %d:", height, width);
        int h = height, w = width;
        if (walk_network<0>(height, width, h, w, &visited)) return 1;
        std::printf("\n");
        if (check_plan(height, width)) return 1;
    }
    // a frame whose first tensors pass 2^31 floats does not fit; one just below does
    CHECK(!vgg_plan(16384, 16384).fits && vgg_plan(4000, 4000).fits && !vgg_plan(4200, 4200).fits, "the 2^31 float bound");
    std::printf("visited %lld\nconv_index_vgg_test: OK\n", visited);
    return 0;
}
