// The SSIM kernel's tile walk (simplenerf_amd/csrc/metrics.hip) on the host, with the kernel's own tile / halo arithmetic
// (csrc/metrics_tile.h): every tile of an h x w image is loaded with its halo into buffers of the kernel's LDS extents, filtered
// along the rows and then the columns, and the S map is written out.  Every buffer is a heap allocation of its exact size
// and every index is checked against its own dimension, so an out-of-range halo / reflect / ragged-tile index aborts (and
// AddressSanitizer / UBSan, which the test builds this with, see the rest).
//   ssim_tile_test <height> <width> <gt.u8> <eval.u8> <s_map.f64>   -> prints "rows: <source row of every (output row, tap)>",
//                                                                      "cols: ...", "ssim_tile_test: OK"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../simplenerf_amd/csrc/metrics_tile.h"

using namespace snerf::ssim_tile;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            std::abort();                                                           \
        }                                                                           \
    } while (0)

static std::vector<unsigned char> read_image(const char* path, size_t bytes) {
    std::vector<unsigned char> data(bytes);
    FILE* f = std::fopen(path, "rb");
    CHECK(f && std::fread(data.data(), 1, bytes, f) == bytes);
    std::fclose(f);
    return data;
}

// source index of every (output position, tap) along one axis, as the tiles of that axis see it
static void print_axis(const char* name, int n, int tile) {
    std::printf("%s:", name);
    for (int origin = 0; origin < n; origin += tile)
        for (int local = 0; local < tile && origin + local < n; ++local)
            for (int k = 0; k < kTaps; ++k) {
                const int s = source_index(origin, local + k, n);
                CHECK(s >= 0 && s < n);
                std::printf(" %d", s);
            }
    std::printf("\n");
}

int main(int argc, char** argv) {
    CHECK(argc == 6);
    const int height = std::atoi(argv[1]), width = std::atoi(argv[2]);
    CHECK(height >= kTaps && width >= kTaps);
    const size_t pixels = (size_t)height * width;
    const std::vector<unsigned char> gt = read_image(argv[3], 3 * pixels), eval = read_image(argv[4], 3 * pixels);
    std::vector<double> s_map(3 * pixels, -1.0);

    double w[kTaps], total = 0.0;
    for (int k = 0; k < kTaps; ++k) total += w[k] = std::exp(-0.5 / (1.5 * 1.5) * (double)((k - kRadius) * (k - kRadius)));
    for (int k = 0; k < kTaps; ++k) w[k] /= total;
    const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);

    for (int y0 = 0; y0 < height; y0 += kTileH)
        for (int x0 = 0; x0 < width; x0 += kTileW) {
            // the kernel's LDS arrays: in_x / in_y [kInH][kInPitch] bytes, rows [5][kInH][kTileW] doubles
            std::vector<unsigned char> in_x((size_t)kInH * kInPitch), in_y((size_t)kInH * kInPitch);
            std::vector<double> rows((size_t)5 * kInH * kTileW);
            for (int i = 0; i < kInH * kInW * 3; ++i) {
                const int r = i / (kInW * 3), b = i - r * (kInW * 3), col = b / 3, c = b - 3 * col;
                const int sy = source_index(y0, r, height), sx = source_index(x0, col, width);
                CHECK(r < kInH && b < kInPitch && sy >= 0 && sy < height && sx >= 0 && sx < width);
                const size_t pixel = (size_t)sy * width + sx;
                in_x.at((size_t)r * kInPitch + b) = gt.at(3 * pixel + c);
                in_y.at((size_t)r * kInPitch + b) = eval.at(3 * pixel + c);
            }
            for (int c = 0; c < 3; ++c) {
                for (int i = 0; i < kInH * kTileW; ++i) {
                    const int r = i / kTileW, col = i - r * kTileW;
                    double m[5] = {0, 0, 0, 0, 0};
                    for (int k = 0; k < kTaps; ++k) {
                        const int b = 3 * (col + k) + c;
                        CHECK(r < kInH && b < 3 * kInW);
                        const double x = in_x.at((size_t)r * kInPitch + b), y = in_y.at((size_t)r * kInPitch + b);
                        m[0] += w[k] * x, m[1] += w[k] * y, m[2] += w[k] * (x * x), m[3] += w[k] * (y * y), m[4] += w[k] * (x * y);
                    }
                    for (int j = 0; j < 5; ++j) rows.at(((size_t)j * kInH + r) * kTileW + col) = m[j];
                }
                for (int oy = 0; oy < kTileH; ++oy)
                    for (int tx = 0; tx < kTileW; ++tx) {
                        double m[5] = {0, 0, 0, 0, 0};
                        for (int k = 0; k < kTaps; ++k) {
                            CHECK(oy + k < kInH);
                            for (int j = 0; j < 5; ++j) m[j] += w[k] * rows.at(((size_t)j * kInH + oy + k) * kTileW + tx);
                        }
                        const int gy = y0 + oy, gx = x0 + tx;
                        if (gy >= height || gx >= width) continue;
                        const double ux = m[0], uy = m[1], vx = m[2] - ux * ux, vy = m[3] - uy * uy, vxy = m[4] - ux * uy;
                        const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2, b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
                        s_map.at(3 * ((size_t)gy * width + gx) + c) = (a1 * a2) / (b1 * b2);
                    }
            }
        }
    FILE* f = std::fopen(argv[5], "wb");
    CHECK(f && std::fwrite(s_map.data(), sizeof(double), s_map.size(), f) == s_map.size());
    std::fclose(f);
    print_axis("rows", height, kTileH);
    print_axis("cols", width, kTileW);
    std::printf("ssim_tile_test: OK\n");
    return 0;
}
