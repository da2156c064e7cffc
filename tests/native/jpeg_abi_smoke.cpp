// The JPEG encoder from the C ABI alone: plain HIP runtime + include/simplenerf_hip.h + csrc/simplenerf_jpeg.h, linked against
// libsimplenerf_hip.so, no PyTorch in the process.
//
//   jpeg_abi_smoke <pixels file> <height> <width> <channels> <quality> <expected scan file>
//
// The frame goes through snerf_jpeg_scan twice in ONE call (two copies: a batch of two), each scan must be the expected file's bytes
// -- tests/test_gpu_jpeg_native.py passes in what the restated encoder gives -- and stay inside snerf_jpeg_scan_bound_bytes; the
// refusals are status codes.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simplenerf_hip.h"
#include "simplenerf_jpeg.h"

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

static bool read_file(const char* path, std::vector<unsigned char>& bytes) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    bytes.resize(size > 0 ? (size_t)size : 0);
    const bool ok = std::fread(bytes.data(), 1, bytes.size(), f) == bytes.size();
    std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 7) return std::printf("usage: jpeg_abi_smoke pixels height width channels quality expected\n"), 1;
    CHECK(snerf_abi_version() == SNERF_ABI_VERSION);
    const int h = std::atoi(argv[2]), w = std::atoi(argv[3]), channels = std::atoi(argv[4]), quality = std::atoi(argv[5]);
    std::vector<unsigned char> frame, expected;
    CHECK(read_file(argv[1], frame) && frame.size() == (size_t)h * w * channels);
    CHECK(read_file(argv[6], expected) && !expected.empty());
    const int images = 2;
    const int mcu = channels == 3 ? 16 : 8;
    const size_t mcus_per_row = (size_t)(w + mcu - 1) / mcu, mcu_rows = (size_t)(h + mcu - 1) / mcu;
    const size_t bound = snerf_jpeg_scan_bound_bytes(h, w, channels);
    CHECK(bound == mcu_rows * (2 * SNERF_JPEG_BLOCK_BYTES * mcus_per_row * (channels == 3 ? 6 : 1) + 2));
    CHECK(expected.size() <= bound);
    const size_t work_bytes = snerf_jpeg_scan_workspace_bytes(images, h, w, channels);
    CHECK(work_bytes >= images * bound);
    CHECK(snerf_jpeg_scan_bound_bytes(h, w, 2) == 0 && snerf_jpeg_scan_bound_bytes(0, w, channels) == 0 &&
          snerf_jpeg_scan_bound_bytes(h, 65536, channels) == 0);
    CHECK(snerf_jpeg_scan_workspace_bytes(0, h, w, channels) == 0 && snerf_jpeg_scan_workspace_bytes(images, h, w, 4) == 0);
    unsigned char *d_pixels = nullptr, *d_scans = nullptr;
    long long* d_sizes = nullptr;
    void* d_work = nullptr;
    HIP_OK(hipMalloc((void**)&d_pixels, images * frame.size()));
    HIP_OK(hipMalloc((void**)&d_scans, images * bound));
    HIP_OK(hipMalloc((void**)&d_sizes, images * sizeof(long long)));
    HIP_OK(hipMalloc(&d_work, work_bytes));
    for (int i = 0; i < images; ++i) HIP_OK(hipMemcpy(d_pixels + i * frame.size(), frame.data(), frame.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_scans, 0xAA, images * bound));
    SNERF_OK_(snerf_jpeg_scan(d_pixels, images, h, w, channels, quality, d_scans, d_sizes, d_work, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<long long> sizes(images);
    std::vector<unsigned char> scans(images * bound);
    HIP_OK(hipMemcpy(sizes.data(), d_sizes, images * sizeof(long long), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(scans.data(), d_scans, scans.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < images; ++i) {
        std::printf("jpeg_abi_smoke: frame %d: %lld scan bytes, expected %zu, bound %zu\n", i, sizes[i], expected.size(), bound);
        CHECK(sizes[i] == (long long)expected.size());
        CHECK(std::memcmp(scans.data() + i * bound, expected.data(), expected.size()) == 0);
        for (size_t k = expected.size(); k < bound; ++k) CHECK(scans[i * bound + k] == 0xAA);          // bytes past the length are not written
    }
    // refusals are status codes, and nothing is enqueued for no images
    CHECK(snerf_jpeg_scan(d_pixels, images, h, w, 2, quality, d_scans, d_sizes, d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_jpeg_scan(d_pixels, images, h, w, channels, 0, d_scans, d_sizes, d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_jpeg_scan(d_pixels, images, h, w, channels, 101, d_scans, d_sizes, d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_jpeg_scan(nullptr, images, h, w, channels, quality, d_scans, d_sizes, d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_jpeg_scan(nullptr, 0, h, w, channels, quality, nullptr, nullptr, nullptr, nullptr) == SNERF_OK);
    HIP_OK(hipFree(d_pixels));
    HIP_OK(hipFree(d_scans));
    HIP_OK(hipFree(d_sizes));
    HIP_OK(hipFree(d_work));
    std::printf("jpeg_abi_smoke: OK\n");
    return 0;
}
