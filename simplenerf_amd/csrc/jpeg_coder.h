// The JPEG encoder's workgroup programs (simplenerf_jpeg.h): transform a chunk of MCUs, emit an MCU row, pack a row.
//
// As in png_coder.h, each program is a sequence of PHASES of a 256-thread workgroup: inside a phase a thread reads only what
// earlier phases wrote (or what it wrote itself) and writes its own slots -- or ORs into shared words, which is order-free -- and a
// workgroup barrier closes every phase.  Control flow between phases is uniform: it depends on the arguments and on shared words
// read after a barrier.  So the same text has a second reading -- a phase is a loop over tid = 0..255 -- which is how a plain C++
// program runs these functions on the host (tests/native/jpeg_coder_host.cpp), under a sanitizer.  Integer arithmetic only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SNERF_JPEG_FN __device__ inline
#define SNERF_JPEG_TABLE static __device__ const
// (`continue` inside a phase body still reaches the barrier; `break` and `return` must not be used there)
#define SNERF_JPEG_PHASE for (int tid = (int)threadIdx.x, phase_once_ = 1; phase_once_; phase_once_ = 0, __syncthreads())
#define SNERF_JPEG_OR(p, v) atomicOr((p), (v))
#else
#define SNERF_JPEG_FN inline
#define SNERF_JPEG_TABLE static const
#define SNERF_JPEG_PHASE for (int tid = 0; tid < snerf::jpeg::kThreads; ++tid)
#define SNERF_JPEG_OR(p, v) (*(p) |= (v))
#endif

namespace snerf {
namespace jpeg {

constexpr int kThreads = 256;
constexpr int kColourChunkMcus = 8, kGreyChunkMcus = 32;      // MCUs one transform workgroup takes: 48 / 32 blocks
constexpr int kChunkBlocks = 48;
constexpr int kBlockBytes = 208;                  // SNERF_JPEG_BLOCK_BYTES: a coded block is at most 22 + 63 * 26 = 1660 bits
constexpr int kBlockWords = kBlockBytes / 4;
constexpr int kPassBlocks = kThreads;             // blocks the emit program codes per pass: one per thread
constexpr int kBitWords = kPassBlocks * kBlockWords + 2;      // 7 carried bits + 256 * 1660 bits, and the word after the last OR

// ITU-T T.81 Annex K.1, in ZIG-ZAG order (as a DQT segment carries them)
SNERF_JPEG_TABLE uint8_t kQuantBase[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101,
     103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// zig-zag index -> 8 * row (vertical frequency) + column (horizontal frequency)
SNERF_JPEG_TABLE uint8_t kZigZag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.3: codes per length 1..16, then the symbols in code order.  Tables 0, 1: DC luminance, chrominance; 2, 3: AC.
SNERF_JPEG_TABLE uint8_t kHuffBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                             {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                             {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                             {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
SNERF_JPEG_TABLE uint8_t kHuffDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
SNERF_JPEG_TABLE uint8_t kHuffAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
// The 1-D DCT-II matrix in 13-bit fixed point: kDct[u][x] = round(8192 * a(u) * cos((2 x + 1) u pi / 16)), a(0) = sqrt(1/8),
// a(u > 0) = 1/2: row 0 is 2896, the others +-{4017, 3784, 3406, 2896, 2276, 1567, 799} = round(4096 cos(k pi / 16)), k = 1..7.
SNERF_JPEG_TABLE int16_t kDct[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},
                                       {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                                       {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},
                                       {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                                       {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},
                                       {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                                       {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},
                                       {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// The quantiser of zig-zag index k of table `table` (0 luminance, 1 chrominance) at `quality` 1..100: the libjpeg rule.
SNERF_JPEG_FN int quantiser(int table, int k, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = (kQuantBase[table][k] * scale + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}

// ------------------------------------------------------------------------------------------------------------ transform
struct TransformShared {
    int32_t v[kChunkBlocks][64];          // samples - 128, then the row pass (x 4), then the column pass (x 8), in place
};

SNERF_JPEG_FN void colour_convert(const uint8_t* p, int& y, int& cb, int& cr) {
    const int r = p[0], g = p[1], b = p[2];
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16;       // 8421375 = 128 * 65536 + 32767: never negative, never above 255
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16;
}

// `mcus` MCUs of MCU row `mcu_row` of one frame, from MCU `first_mcu` on -> their blocks' quantised coefficients in zig-zag order,
// 64 int16 per block, blocks in scan order (colour: Y00 Y01 Y10 Y11 Cb Cr per MCU), at `out`.
SNERF_JPEG_FN void transform_chunk(TransformShared& sh, const uint8_t* frame, int height, int width, int channels, int quality,
                                   int mcu_row, int first_mcu, int mcus, int16_t* out) {
    const int blocks = channels == 3 ? 6 * mcus : mcus;
    SNERF_JPEG_PHASE {
        if (channels == 3) {
            // a thread per 2 x 2 cell: four luminance samples, one sample of each chrominance plane
            for (int c = tid; c < mcus * 64; c += kThreads) {
                const int m = c >> 6, cy = (c >> 3) & 7, cx = c & 7;
                int sum_cb = 0, sum_cr = 0;
                for (int d = 0; d < 4; ++d) {
                    const int my = 2 * cy + (d >> 1), mx = 2 * cx + (d & 1);              // inside the MCU
                    int py = mcu_row * 16 + my, px = (first_mcu + m) * 16 + mx;
                    py = py < height ? py : height - 1;                                   // the last row and column repeat
                    px = px < width ? px : width - 1;
                    int y, cb, cr;
                    colour_convert(frame + ((size_t)py * width + px) * 3, y, cb, cr);
                    sh.v[m * 6 + (my >> 3) * 2 + (mx >> 3)][(my & 7) * 8 + (mx & 7)] = y - 128;
                    sum_cb += cb;
                    sum_cr += cr;
                }
                sh.v[m * 6 + 4][cy * 8 + cx] = ((sum_cb + 2) >> 2) - 128;
                sh.v[m * 6 + 5][cy * 8 + cx] = ((sum_cr + 2) >> 2) - 128;
            }
        } else {
            for (int c = tid; c < mcus * 64; c += kThreads) {
                const int m = c >> 6, my = (c >> 3) & 7, mx = c & 7;
                int py = mcu_row * 8 + my, px = (first_mcu + m) * 8 + mx;
                py = py < height ? py : height - 1;
                px = px < width ? px : width - 1;
                sh.v[m][my * 8 + mx] = (int)frame[(size_t)py * width + px] - 128;
            }
        }
    }
    SNERF_JPEG_PHASE {          // rows: t[y][u] = (sum_x kDct[u][x] s[y][x] + 2^10) >> 11  -- four times the 1-D transform
        for (int t = tid; t < blocks * 8; t += kThreads) {
            int32_t* row = &sh.v[t >> 3][(t & 7) * 8];
            int32_t s[8];
            for (int x = 0; x < 8; ++x) s[x] = row[x];
            for (int u = 0; u < 8; ++u) {
                int32_t sum = 1 << 10;
                for (int x = 0; x < 8; ++x) sum += kDct[u][x] * s[x];
                row[u] = sum >> 11;
            }
        }
    }
    SNERF_JPEG_PHASE {          // columns: F8[v][u] = (sum_y kDct[v][y] t[y][u] + 2^11) >> 12  -- eight times the 2-D transform
        for (int t = tid; t < blocks * 8; t += kThreads) {
            int32_t* column = &sh.v[t >> 3][t & 7];
            int32_t s[8];
            for (int y = 0; y < 8; ++y) s[y] = column[8 * y];
            for (int v = 0; v < 8; ++v) {
                int32_t sum = 1 << 11;
                for (int y = 0; y < 8; ++y) sum += kDct[v][y] * s[y];
                column[8 * v] = sum >> 12;
            }
        }
    }
    SNERF_JPEG_PHASE {          // quantise: round(|F8| / (8 q)), half away from zero, with the sign of F8; zig-zag order
        for (int t = tid; t < blocks * 64; t += kThreads) {
            const int block = t >> 6, k = t & 63;
            const int table = channels == 3 && block % 6 >= 4;
            const int q = quantiser(table, k, quality);
            const int f = sh.v[block][kZigZag[k]];
            int level = ((f < 0 ? -f : f) + 4 * q) / (8 * q);
            const int limit = k == 0 && f < 0 ? 1024 : 1023;          // (8-bit samples stay inside it: it is there for the bit bound)
            level = level > limit ? limit : level;
            out[(size_t)block * 64 + k] = (int16_t)(f < 0 ? -level : level);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ emit
struct EmitShared {
    uint32_t bits[kBitWords];             // big-endian: stream bit p is bit 31 - (p & 31) of word p >> 5
    uint32_t count[kThreads], offset[kThreads];
    uint16_t ac_code[2][256], dc_code[2][12];
    uint8_t ac_len[2][256], dc_len[2][12];
    uint32_t total;                       // bits in the buffer: the carried ones and this pass's
    uint32_t carry_bits, carry_byte;      // the 0..7 bits of the last pass that did not fill a byte, in the top of a byte
    uint32_t written;                     // bytes of the row written so far
};

SNERF_JPEG_FN int magnitude_size(int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// The symbols of one block, in order: f.put(bits, length), 1 <= length <= 26, most significant bit first.
template <class F>
SNERF_JPEG_FN void code_block(const EmitShared& sh, const int16_t* c, int predictor, int table, F& f) {
    const int diff = c[0] - predictor;
    int size = magnitude_size(diff);
    f.put(((uint32_t)sh.dc_code[table][size] << size) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1)),
          sh.dc_len[table][size] + size);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = c[k];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run >= 16; run -= 16) f.put(sh.ac_code[table][0xF0], sh.ac_len[table][0xF0]);          // ZRL
        size = magnitude_size(v);
        const int symbol = run << 4 | size;
        f.put(((uint32_t)sh.ac_code[table][symbol] << size) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1)),
              sh.ac_len[table][symbol] + size);
        run = 0;
    }
    if (run) f.put(sh.ac_code[table][0], sh.ac_len[table][0]);          // EOB: not after a non-zero 63rd coefficient
}

struct CountBits {
    uint32_t bits;
    SNERF_JPEG_FN void put(uint32_t, int length) { bits += (uint32_t)length; }
};

struct WriteBits {
    uint32_t* words;
    uint32_t at;
    SNERF_JPEG_FN void put(uint32_t value, int length) {
        const int inside = (int)(at & 31);
        const uint64_t placed = (uint64_t)value << (64 - inside - length);          // inside + length <= 57
        SNERF_JPEG_OR(&words[at >> 5], (uint32_t)(placed >> 32));
        if (inside + length > 32) SNERF_JPEG_OR(&words[(at >> 5) + 1], (uint32_t)placed);
        at += (uint32_t)length;
    }
};

// block b of an MCU row -> its Huffman table pair (0 luminance, 1 chrominance) and the block whose DC predicts its own (-1: none)
SNERF_JPEG_FN void block_place(int b, int colour, int& table, int& before) {
    if (!colour) {
        table = 0, before = b - 1;
        return;
    }
    const int part = b % 6;
    table = part >= 4;
    before = part >= 4 ? b - 6 : (part ? b - 1 : b - 3);          // Cb, Cr: the MCU before; Y00: the Y11 before
}

SNERF_JPEG_FN uint32_t buffer_byte(const EmitShared& sh, uint32_t k, uint32_t padded_at, uint32_t pad) {
    const uint32_t v = (sh.bits[k >> 2] >> (24 - 8 * (k & 3))) & 255u;
    return k == padded_at ? v | pad : v;
}

// One MCU row: `blocks` blocks of coefficients at `coefs` -> its entropy-coded bytes at `out` (stuffed, padded with 1-bits, then
// FF D0+restart unless restart < 0: the frame's last row), their number in *out_bytes.  At most 2 * kBlockBytes * blocks + 2 bytes.
SNERF_JPEG_FN void emit_row(EmitShared& sh, const int16_t* coefs, int blocks, int colour, int restart, uint8_t* out, int* out_bytes) {
    SNERF_JPEG_PHASE {
        if (tid < 4) {          // the canonical codes of Annex C from the four tables
            const uint8_t* vals = tid < 2 ? kHuffDcVals : kHuffAcVals[tid - 2];
            uint32_t code = 0;
            int at = 0;
            for (int length = 1; length <= 16; ++length) {
                for (int i = 0; i < kHuffBits[tid][length - 1]; ++i, ++at, ++code) {
                    if (tid < 2) {
                        sh.dc_code[tid][vals[at]] = (uint16_t)code, sh.dc_len[tid][vals[at]] = (uint8_t)length;
                    } else {
                        sh.ac_code[tid - 2][vals[at]] = (uint16_t)code, sh.ac_len[tid - 2][vals[at]] = (uint8_t)length;
                    }
                }
                code <<= 1;
            }
        }
        if (tid == 0) sh.carry_bits = 0, sh.carry_byte = 0, sh.written = 0;
    }
    for (int first = 0; first < blocks; first += kPassBlocks) {
        const bool last = first + kPassBlocks >= blocks;
        SNERF_JPEG_PHASE {
            const int b = first + tid;
            CountBits counter{0};
            if (b < blocks) {
                int table, before;
                block_place(b, colour, table, before);
                code_block(sh, coefs + (size_t)b * 64, before >= 0 ? coefs[(size_t)before * 64] : 0, table, counter);
            }
            sh.count[tid] = counter.bits;
        }
        SNERF_JPEG_PHASE {
            if (tid == 0) {
                uint32_t run = sh.carry_bits;
                for (int i = 0; i < kThreads; ++i) {
                    sh.offset[i] = run;
                    run += sh.count[i];
                }
                sh.total = run;
            }
        }
        const uint32_t total = sh.total, words = (total + 31) / 32 + 1;
        SNERF_JPEG_PHASE {
            for (uint32_t i = (uint32_t)tid; i < words; i += kThreads) sh.bits[i] = i ? 0u : sh.carry_byte << 24;
        }
        SNERF_JPEG_PHASE {
            const int b = first + tid;
            if (b < blocks) {
                int table, before;
                block_place(b, colour, table, before);
                WriteBits writer{sh.bits, sh.offset[tid]};
                code_block(sh, coefs + (size_t)b * 64, before >= 0 ? coefs[(size_t)before * 64] : 0, table, writer);
            }
        }
        // whole bytes leave; the row's last pass pads its open byte with 1-bits and it leaves too
        const uint32_t open = total & 7, padded = last && open;
        const uint32_t flush = (total >> 3) + (padded ? 1u : 0u);
        const uint32_t padded_at = padded ? total >> 3 : 0xffffffffu, pad = (1u << (8 - open)) - 1;
        const uint32_t each = (flush + kThreads - 1) / kThreads;
        SNERF_JPEG_PHASE {
            const uint32_t from = (uint32_t)tid * each, to = from + each < flush ? from + each : flush;
            uint32_t stuffed = 0;
            for (uint32_t k = from; k < to; ++k) stuffed += buffer_byte(sh, k, padded_at, pad) == 255u;
            sh.count[tid] = stuffed;
        }
        SNERF_JPEG_PHASE {
            if (tid == 0) {
                uint32_t run = sh.written;
                for (int i = 0; i < kThreads; ++i) {
                    const uint32_t from = (uint32_t)i * each, to = from + each < flush ? from + each : flush;
                    sh.offset[i] = run;
                    run += (to > from ? to - from : 0u) + sh.count[i];
                }
                sh.written = run;
                sh.carry_bits = last ? 0u : open;
                sh.carry_byte = last ? 0u : buffer_byte(sh, total >> 3, padded_at, pad);
            }
        }
        SNERF_JPEG_PHASE {
            const uint32_t from = (uint32_t)tid * each, to = from + each < flush ? from + each : flush;
            uint8_t* at = out + sh.offset[tid];
            for (uint32_t k = from; k < to; ++k) {
                const uint32_t v = buffer_byte(sh, k, padded_at, pad);
                *at++ = (uint8_t)v;
                if (v == 255u) *at++ = 0;
            }
        }
    }
    SNERF_JPEG_PHASE {
        if (tid == 0) {
            uint32_t written = sh.written;
            if (restart >= 0) {
                out[written++] = 0xFF;
                out[written++] = (uint8_t)(0xD0 + restart);
            }
            *out_bytes = (int)written;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ pack
struct PackShared {
    unsigned long long sums[kThreads];
    unsigned long long offset;
};

// Row `row` of a frame of `rows` MCU rows: its bytes go behind those of the rows before it; the last row reports the length.
SNERF_JPEG_FN void pack_row(PackShared& sh, const int* sizes, int row, int rows, const uint8_t* slot, uint8_t* scan, long long* scan_bytes) {
    SNERF_JPEG_PHASE {
        unsigned long long sum = 0;
        for (int r = tid; r < row; r += kThreads) sum += (unsigned long long)sizes[r];
        sh.sums[tid] = sum;
    }
    SNERF_JPEG_PHASE {
        if (tid == 0) {
            unsigned long long total = 0;
            for (int i = 0; i < kThreads; ++i) total += sh.sums[i];
            sh.offset = total;
            if (row == rows - 1) *scan_bytes = (long long)(total + (unsigned long long)sizes[row]);
        }
    }
    SNERF_JPEG_PHASE {
        uint8_t* to = scan + sh.offset;
        for (int i = tid; i < sizes[row]; i += kThreads) to[i] = slot[i];
    }
}

}  // namespace jpeg
}  // namespace snerf
