// The PNG encoder's workgroup programs (simplenerf_amd/csrc/png_coder.h) run on the host: a phase is a loop over the 256 threads.
// The same buffers, sizes and offsets as snerf_png_deflate (csrc/png.hip), so that every index the kernels form is formed here
// first -- build with -fsanitize=address,undefined.
//
//   png_coder_host <pixels file> <images> <height> <width> <channels> <filter_mode> <streams file>
//
// reads images * height * width * channels bytes and writes, per image, an 8-byte little-endian stream length and the stream.
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>

#include "../../simplenerf_amd/csrc/png_coder.h"

using namespace snerf::png;

int main(int argc, char** argv) {
    if (argc != 8) return std::fprintf(stderr, "usage: png_coder_host pixels images height width channels filter_mode streams\n"), 2;
    const int images = std::atoi(argv[2]), height = std::atoi(argv[3]), width = std::atoi(argv[4]), channels = std::atoi(argv[5]);
    const int mode = std::atoi(argv[6]);
    const int row_bytes = width * channels, raw = height * (1 + row_bytes);
    const int strips = (raw + kStrip - 1) / kStrip;
    const size_t bound = (size_t)raw + 5 * (size_t)strips + 6, stride = ((size_t)raw + 15) / 16 * 16;
    // exact sizes, so that the sanitizer sees every byte past an end
    std::vector<uint8_t> pixels((size_t)images * height * row_bytes);
    FILE* in = std::fopen(argv[1], "rb");
    if (!in || std::fread(pixels.data(), 1, pixels.size(), in) != pixels.size()) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    std::fclose(in);
    std::vector<uint8_t> filtered_bytes(images * stride), streams(images * bound, 0xAA);
    uint8_t* slots = static_cast<uint8_t*>(::operator new((size_t)images * strips * kSlot, std::align_val_t(16)));
    std::vector<int> sizes((size_t)images * strips);
    std::vector<uint32_t> adler((size_t)images * strips * 2);
    std::vector<long long> offsets((size_t)images * strips), stream_bytes(images);
    auto* filter_shared = new FilterShared;
    auto* strip_shared = new StripShared;
    auto* scan_shared = new ScanShared;
    for (int i = 0; i < images; ++i) {
        for (int y = 0; y < height; ++y) {
            const uint8_t* cur = pixels.data() + ((size_t)i * height + y) * row_bytes;
            filter_row(*filter_shared, cur, y ? cur - row_bytes : nullptr, row_bytes, channels, mode,
                       filtered_bytes.data() + i * stride + (size_t)y * (1 + row_bytes));
        }
        for (int s = 0; s < strips; ++s) {
            const int length = raw - s * kStrip < kStrip ? raw - s * kStrip : kStrip;
            encode_strip(*strip_shared, filtered_bytes.data() + i * stride + (size_t)s * kStrip, length, s == strips - 1,
                         slots + ((size_t)i * strips + s) * kSlot, &sizes[(size_t)i * strips + s], &adler[((size_t)i * strips + s) * 2]);
        }
        scan_frame(*scan_shared, &sizes[(size_t)i * strips], &adler[(size_t)i * strips * 2], strips, raw, &offsets[(size_t)i * strips],
                   streams.data() + i * bound, &stream_bytes[i]);
        for (int s = 0; s < strips; ++s)
            pack_strip(slots + ((size_t)i * strips + s) * kSlot, sizes[(size_t)i * strips + s],
                       streams.data() + i * bound + offsets[(size_t)i * strips + s]);
        if (stream_bytes[i] > (long long)bound) return std::fprintf(stderr, "image %d: %lld bytes > bound %zu\n", i, stream_bytes[i], bound), 1;
    }
    FILE* out = std::fopen(argv[7], "wb");
    if (!out) return std::fprintf(stderr, "cannot write %s\n", argv[7]), 2;
    for (int i = 0; i < images; ++i) {
        const unsigned long long n = (unsigned long long)stream_bytes[i];
        uint8_t le[8];
        for (int k = 0; k < 8; ++k) le[k] = (uint8_t)(n >> (8 * k));
        std::fwrite(le, 1, 8, out);
        std::fwrite(streams.data() + i * bound, 1, (size_t)n, out);
    }
    std::fclose(out);
    ::operator delete(slots, std::align_val_t(16));
    delete filter_shared;
    delete strip_shared;
    delete scan_shared;
    return 0;
}
