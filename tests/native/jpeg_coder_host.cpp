// The JPEG encoder's workgroup programs (simplenerf_amd/csrc/jpeg_coder.h) run on the host: a phase is a loop over the 256 threads.
// The same buffers, sizes and offsets as snerf_jpeg_scan (csrc/jpeg.hip), so that every index the kernels form is formed here
// first -- build with -fsanitize=address,undefined.
//
//   jpeg_coder_host <pixels file> <images> <height> <width> <channels> <quality> <scans file>
//
// reads images * height * width * channels bytes and writes, per image, an 8-byte little-endian scan length and the scan.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../simplenerf_amd/csrc/jpeg_coder.h"

using namespace snerf::jpeg;

int main(int argc, char** argv) {
    if (argc != 8) return std::fprintf(stderr, "usage: jpeg_coder_host pixels images height width channels quality scans\n"), 2;
    const int images = std::atoi(argv[2]), height = std::atoi(argv[3]), width = std::atoi(argv[4]), channels = std::atoi(argv[5]);
    const int quality = std::atoi(argv[6]);
    const int mcu = channels == 3 ? 16 : 8, per_mcu = channels == 3 ? 6 : 1;
    const int mcus_per_row = (width + mcu - 1) / mcu, mcu_rows = (height + mcu - 1) / mcu, blocks_per_row = mcus_per_row * per_mcu;
    const int chunk_mcus = channels == 3 ? kColourChunkMcus : kGreyChunkMcus;
    const size_t row_bound = 2 * (size_t)kBlockBytes * blocks_per_row + 2, bound = mcu_rows * row_bound;
    // exact sizes, so that the sanitizer sees every byte past an end
    std::vector<uint8_t> pixels((size_t)images * height * width * channels);
    FILE* in = std::fopen(argv[1], "rb");
    if (!in || std::fread(pixels.data(), 1, pixels.size(), in) != pixels.size()) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    std::fclose(in);
    std::vector<int16_t> levels((size_t)images * mcu_rows * blocks_per_row * 64);
    std::vector<uint8_t> slots((size_t)images * mcu_rows * row_bound), scans(images * bound, 0xAA);
    std::vector<int> sizes((size_t)images * mcu_rows);
    std::vector<long long> scan_bytes(images);
    auto* transform_shared = new TransformShared;
    auto* emit_shared = new EmitShared;
    auto* pack_shared = new PackShared;
    for (int i = 0; i < images; ++i) {
        const uint8_t* frame = pixels.data() + (size_t)i * height * width * channels;
        for (int r = 0; r < mcu_rows; ++r) {
            const size_t row = (size_t)i * mcu_rows + r;
            for (int first = 0; first < mcus_per_row; first += chunk_mcus) {
                const int left = mcus_per_row - first;
                transform_chunk(*transform_shared, frame, height, width, channels, quality, r, first, left < chunk_mcus ? left : chunk_mcus,
                                levels.data() + (row * blocks_per_row + (size_t)first * per_mcu) * 64);
            }
            emit_row(*emit_shared, levels.data() + row * blocks_per_row * 64, blocks_per_row, channels == 3, r == mcu_rows - 1 ? -1 : r & 7,
                     slots.data() + row * row_bound, &sizes[row]);
            if ((size_t)sizes[row] > row_bound) return std::fprintf(stderr, "row %d: %d bytes > bound %zu\n", r, sizes[row], row_bound), 1;
        }
        for (int r = 0; r < mcu_rows; ++r)
            pack_row(*pack_shared, &sizes[(size_t)i * mcu_rows], r, mcu_rows, slots.data() + ((size_t)i * mcu_rows + r) * row_bound,
                     scans.data() + i * bound, &scan_bytes[i]);
    }
    FILE* out = std::fopen(argv[7], "wb");
    if (!out) return std::fprintf(stderr, "cannot write %s\n", argv[7]), 2;
    for (int i = 0; i < images; ++i) {
        const unsigned long long n = (unsigned long long)scan_bytes[i];
        uint8_t le[8];
        for (int k = 0; k < 8; ++k) le[k] = (uint8_t)(n >> (8 * k));
        std::fwrite(le, 1, 8, out);
        std::fwrite(scans.data() + i * bound, 1, (size_t)n, out);
    }
    std::fclose(out);
    delete transform_shared;
    delete emit_shared;
    delete pack_shared;
    return 0;
}
