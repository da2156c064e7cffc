// Walks simplenerf_amd/csrc/conv_index.h on the host (built with -fsanitize=address,undefined by tests/test_lpips_host.py): for
// every image extent given on the command line ("h w" pairs) and every layer it
//   * checks the output extents against the closed forms floor((in + 2 pad - k) / stride) + 1 and floor((in - 3) / 2) + 1,
//   * enumerates every (output pixel, k) of the implicit GEMM and compares k's tap and the source coordinate / padding predicate
//     with a direct triple loop over (tap row, tap column, channel), touching the source tensor at every in-range coordinate (a
//     wrong index is an out-of-bounds access the sanitizer reports) and counting that every source element a tap can reach is hit,
//   * checks that every pool window lies inside its source and that the windows cover it up to the floor-mode remainder.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../simplenerf_amd/csrc/conv_index.h"

using namespace snerf::conv_index;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("conv_index_test: FAILED %s: ", #cond); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            return 1;                                     \
        }                                                 \
    } while (0)

static int closed_conv(int in, int k, int stride, int pad) { return (int)std::floor((double)(in + 2 * pad - k) / stride) + 1; }
static int closed_pool(int in) { return (int)std::floor((double)(in - 3) / 2) + 1; }

static int walk_pool(int in_h, int in_w) {
    const int out_h = pool_extent(in_h), out_w = pool_extent(in_w);
    CHECK(out_h == closed_pool(in_h) && out_w == closed_pool(in_w) && out_h >= 1 && out_w >= 1, "pool of %d x %d", in_h, in_w);
    std::vector<unsigned char> seen((size_t)in_h * in_w, 0);
    for (int oy = 0; oy < out_h; ++oy)
        for (int ox = 0; ox < out_w; ++ox)
            for (int dy = 0; dy < kPoolWindow; ++dy)
                for (int dx = 0; dx < kPoolWindow; ++dx) {
                    const int y = pool_first(oy) + dy, x = pool_first(ox) + dx;
                    CHECK(y >= 0 && y < in_h && x >= 0 && x < in_w, "pool window (%d, %d) + (%d, %d) leaves %d x %d", oy, ox, dy, dx, in_h, in_w);
                    seen[(size_t)y * in_w + x] = 1;
                }
    // floor mode: rows / columns beyond the last window (at most one) are never read, everything before is
    for (int y = 0; y < in_h; ++y)
        for (int x = 0; x < in_w; ++x) {
            const bool covered = y <= pool_first(out_h - 1) + kPoolWindow - 1 && x <= pool_first(out_w - 1) + kPoolWindow - 1;
            CHECK(seen[(size_t)y * in_w + x] == (covered ? 1 : 0), "pool coverage at (%d, %d) of %d x %d", y, x, in_h, in_w);
        }
    CHECK(in_h - (pool_first(out_h - 1) + kPoolWindow) <= 1 && in_w - (pool_first(out_w - 1) + kPoolWindow) <= 1, "pool remainder");
    return 0;
}

static int walk_conv(const ConvGeom& g, int in_h, int in_w, long long* visited) {
    const int out_h = conv_extent(in_h, g), out_w = conv_extent(in_w, g);
    CHECK(out_h == closed_conv(in_h, g.kernel, g.stride, g.pad) && out_w == closed_conv(in_w, g.kernel, g.stride, g.pad), "conv extents");
    CHECK(out_h >= 1 && out_w >= 1, "empty output for %d x %d", in_h, in_w);
    CHECK(k_count(g) == g.kernel * g.kernel * g.c_in && k_padded(g) % kSlab == 0 && k_padded(g) >= k_count(g) &&
              k_padded(g) - k_count(g) < kSlab, "k padding");
    std::vector<unsigned char> source((size_t)in_h * in_w * g.c_in, 0);     // touched through the header's indices
    for (int oy = 0; oy < out_h; ++oy)
        for (int ox = 0; ox < out_w; ++ox) {
            int k = 0;
            for (int ky = 0; ky < g.kernel; ++ky)
                for (int kx = 0; kx < g.kernel; ++kx)
                    for (int c = 0; c < g.c_in; ++c, ++k) {
                        const Tap t = k_tap(g, k);
                        CHECK(t.ky == ky && t.kx == kx && t.c == c && k_index(g, ky, kx, c) == k, "k %d -> (%d, %d, %d)", k, t.ky, t.kx, t.c);
                        const int iy = source_origin(g, oy) + t.ky, ix = source_origin(g, ox) + t.kx;
                        CHECK(iy == oy * g.stride - g.pad + ky && ix == ox * g.stride - g.pad + kx, "source of (%d, %d) tap (%d, %d)", oy, ox, ky, kx);
                        const bool inside = in_source(iy, in_h) && in_source(ix, in_w);
                        CHECK(inside == (iy >= 0 && iy < in_h && ix >= 0 && ix < in_w), "padding predicate at (%d, %d)", iy, ix);
                        if (inside) source[((size_t)iy * in_w + ix) * g.c_in + t.c] = 1;
                        ++*visited;
                    }
            CHECK(k == k_count(g), "k count");
        }
    // every source element that some output's window reaches was touched: rows / columns up to the last window's end
    const int last_y = source_origin(g, out_h - 1) + g.kernel - 1, last_x = source_origin(g, out_w - 1) + g.kernel - 1;
    for (int y = 0; y < in_h; ++y)
        for (int x = 0; x < in_w; ++x)
            for (int c = 0; c < g.c_in; ++c) {
                const bool reachable = y <= last_y && x <= last_x && (g.stride <= g.kernel);
                CHECK(source[((size_t)y * in_w + x) * g.c_in + c] == (reachable ? 1 : 0), "source coverage at (%d, %d, %d)", y, x, c);
            }
    return 0;
}

int main(int argc, char** argv) {
    CHECK(argc >= 3 && argc % 2 == 1, "usage: conv_index_test h w [h w ...]");
    CHECK(kLayers == 5 && kGeom[0].c_in == 3 && kGeom[4].c_out == 256, "geometry table");
    for (int l = 0; l + 1 < kLayers; ++l) CHECK(kGeom[l].c_out == kGeom[l + 1].c_in, "channels of layer %d", l);
    for (int l = 0; l < kLayers; ++l) CHECK(kGeom[l].c_out % 64 == 0, "c_out of layer %d", l);
    CHECK(tap_extent(kMinExtent, 4) == 1 && tap_extent(kMinExtent - 1, 4) == 0 && tap_extent(kMinExtent, 0) == 7, "minimum extent");
    long long visited = 0;
    for (int arg = 1; arg + 1 < argc; arg += 2) {
        const int height = std::atoi(argv[arg]), width = std::atoi(argv[arg + 1]);
        CHECK(height >= kMinExtent && width >= kMinExtent, "extent %d x %d", height, width);
        int h = height, w = width;
        std::printf("extents %d x %d:", height, width);
        for (int l = 0; l < kLayers; ++l) {
            if (kGeom[l].pool_before) {
                if (walk_pool(h, w)) return 1;
                h = pool_extent(h);
                w = pool_extent(w);
            }
            if (walk_conv(kGeom[l], h, w, &visited)) return 1;
            h = conv_extent(h, kGeom[l]);
            w = conv_extent(w, kGeom[l]);
            CHECK(h == tap_extent(height, l) && w == tap_extent(width, l), "tap_extent of layer %d", l);
            std::printf(" %d x %d", h, w);
        }
        std::printf("\n");
    }
    std::printf("visited %lld\nconv_index_test: OK\n", visited);
    return 0;
}
