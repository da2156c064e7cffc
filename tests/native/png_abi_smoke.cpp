// The PNG encoder from the C ABI alone: plain HIP runtime + include/simplenerf_hip.h + csrc/simplenerf_png.h, linked against
// libsimplenerf_hip.so, no PyTorch in the process.  Three RGB frames of 40 x 61 (a ramp with seeded noise, a flat one, pure noise)
// in ONE snerf_png_deflate call and one grey 70 x 500 ramp (35 070 filtered bytes: two strips) in a second; each stream is wrapped
// in the PNG container here, with a table CRC-32 of this file's own, and written to <directory>/<name>_<h>x<w>x<c>.png beside
// the pixels (<same name>.raw).  tests/test_gpu_png_native.py builds and runs the program and decodes the files.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "simplenerf_hip.h"
#include "simplenerf_png.h"

#define HIP_OK(x)                                                                      \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) { std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 2; } \
    } while (0)
#define SNERF_OK_(x)                                                                   \
    do {                                                                               \
        if ((x) != 0) { std::printf("ABI error at %s:%d: %s\n", __FILE__, __LINE__, snerf_last_error()); return 3; } \
    } while (0)
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::printf("check failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); return 4; } \
    } while (0)

static unsigned crc_table[256];

static unsigned crc32(const std::vector<unsigned char>& bytes) {
    unsigned crc = 0xffffffffu;
    for (unsigned char b : bytes) crc = crc_table[(crc ^ b) & 255] ^ (crc >> 8);
    return crc ^ 0xffffffffu;
}

static void big_endian(std::vector<unsigned char>& to, unsigned v) {
    for (int shift = 24; shift >= 0; shift -= 8) to.push_back((unsigned char)(v >> shift));
}

static void chunk(std::vector<unsigned char>& file, const char* tag, const std::vector<unsigned char>& data) {
    std::vector<unsigned char> body(tag, tag + 4);
    body.insert(body.end(), data.begin(), data.end());
    big_endian(file, (unsigned)data.size());
    file.insert(file.end(), body.begin(), body.end());
    big_endian(file, crc32(body));
}

static bool write_file(const std::string& path, const std::vector<unsigned char>& bytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    return std::fclose(f) == 0 && ok;
}

// images of one shape through one call; files named <names[i]>_<h>x<w>x<c>
static int encode(const std::string& directory, const std::vector<std::string>& names, const std::vector<unsigned char>& pixels, int h,
                  int w, int channels, int filter_mode) {
    const int images = (int)names.size();
    const size_t bound = snerf_png_deflate_bound_bytes(h, w, channels), raw = (size_t)h * (1 + (size_t)w * channels);
    CHECK(bound >= raw + 6 && bound <= raw + 10 * ((raw + SNERF_PNG_STRIP_BYTES - 1) / SNERF_PNG_STRIP_BYTES) + 6);
    const size_t work_bytes = snerf_png_deflate_workspace_bytes(images, h, w, channels);
    CHECK(work_bytes > 0);
    unsigned char *d_pixels = nullptr, *d_streams = nullptr;
    long long* d_sizes = nullptr;
    void* d_work = nullptr;
    HIP_OK(hipMalloc((void**)&d_pixels, pixels.size()));
    HIP_OK(hipMalloc((void**)&d_streams, images * bound));
    HIP_OK(hipMalloc((void**)&d_sizes, images * sizeof(long long)));
    HIP_OK(hipMalloc(&d_work, work_bytes));
    HIP_OK(hipMemcpy(d_pixels, pixels.data(), pixels.size(), hipMemcpyHostToDevice));
    SNERF_OK_(snerf_png_deflate(d_pixels, images, h, w, channels, filter_mode, d_streams, d_sizes, d_work, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<long long> sizes(images);
    std::vector<unsigned char> streams(images * bound);
    HIP_OK(hipMemcpy(sizes.data(), d_sizes, images * sizeof(long long), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(streams.data(), d_streams, streams.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < images; ++i) {
        CHECK(sizes[i] >= 8 && (size_t)sizes[i] <= bound);
        std::vector<unsigned char> file = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'}, header;
        big_endian(header, (unsigned)w);
        big_endian(header, (unsigned)h);
        const unsigned char rest[5] = {8, (unsigned char)(channels == 3 ? 2 : 0), 0, 0, 0};
        header.insert(header.end(), rest, rest + 5);
        chunk(file, "IHDR", header);
        chunk(file, "IDAT", std::vector<unsigned char>(streams.begin() + i * bound, streams.begin() + i * bound + sizes[i]));
        chunk(file, "IEND", {});
        const std::string stem = directory + "/" + names[i] + "_" + std::to_string(h) + "x" + std::to_string(w) + "x" + std::to_string(channels);
        const size_t frame = (size_t)h * w * channels;
        CHECK(write_file(stem + ".png", file));
        CHECK(write_file(stem + ".raw", std::vector<unsigned char>(pixels.begin() + i * frame, pixels.begin() + (i + 1) * frame)));
        std::printf("png_abi_smoke: %s %lld stream bytes of %zu raw\n", stem.c_str(), sizes[i], raw);
    }
    // refusals are status codes, and nothing is enqueued for no images
    CHECK(snerf_png_deflate(d_pixels, images, h, w, 2, filter_mode, d_streams, d_sizes, d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_png_deflate(d_pixels, images, h, w, channels, 5, d_streams, d_sizes, d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_png_deflate(nullptr, images, h, w, channels, filter_mode, d_streams, d_sizes, d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_png_deflate(nullptr, 0, h, w, channels, filter_mode, nullptr, nullptr, nullptr, nullptr) == SNERF_OK);
    HIP_OK(hipFree(d_pixels));
    HIP_OK(hipFree(d_streams));
    HIP_OK(hipFree(d_sizes));
    HIP_OK(hipFree(d_work));
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return std::printf("usage: png_abi_smoke <directory>\n"), 1;
    CHECK(snerf_abi_version() == SNERF_ABI_VERSION);
    for (unsigned n = 0; n < 256; ++n) {
        unsigned c = n;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
        crc_table[n] = c;
    }
    unsigned state = 77u;
    auto draw = [&state]() {
        state = state * 1664525u + 1013904223u;
        return state >> 24;
    };
    const int h = 40, w = 61;
    std::vector<unsigned char> colour((size_t)3 * h * w * 3);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < 3; ++c) {
                const size_t at = ((size_t)y * w + x) * 3 + c, frame = (size_t)h * w * 3;
                colour[at] = (unsigned char)((3 * x + 2 * y + 40 * c + (draw() & 3)) & 255);
                colour[frame + at] = 200;
                colour[2 * frame + at] = (unsigned char)draw();
            }
    int status = encode(argv[1], {"ramp", "flat", "noise"}, colour, h, w, 3, SNERF_PNG_FILTER_ADAPTIVE);
    if (status) return status;
    const int gh = 70, gw = 500;
    std::vector<unsigned char> grey((size_t)gh * gw);
    for (int y = 0; y < gh; ++y)
        for (int x = 0; x < gw; ++x) grey[(size_t)y * gw + x] = (unsigned char)((x / 2 + y + (draw() & 1)) & 255);
    status = encode(argv[1], {"grey"}, grey, gh, gw, 1, SNERF_PNG_FILTER_ADAPTIVE);
    if (status) return status;
    status = encode(argv[1], {"grey_up"}, grey, gh, gw, 1, 2);
    if (status) return status;
    std::printf("png_abi_smoke: OK\n");
    return 0;
}
