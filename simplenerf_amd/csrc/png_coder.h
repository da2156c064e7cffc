// The PNG encoder's workgroup programs (simplenerf_png.h): filter a row, code a strip, scan a frame's strip sizes, pack a strip.
//
// Each program is a sequence of PHASES of a 256-thread workgroup: inside a phase a thread reads only what earlier phases wrote (or
// what it wrote itself) and writes its own slots -- or adds / ORs into shared words, which is order-free -- and a workgroup barrier
// closes every phase.  Control flow between phases is uniform: it depends on kernel arguments and on shared words read after a
// barrier.  Written that way the same text has a second reading -- a phase is a loop over tid = 0..255 -- which is how a plain C++
// program runs these functions on the host (tests/native/png_coder_host.cpp): every index below can be checked there, with a
// sanitizer, before it runs on a device.  Integer arithmetic only.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SNERF_PNG_FN __device__ inline
// (`continue` inside a phase body still reaches the barrier; `break` and `return` must not be used there)
#define SNERF_PNG_PHASE for (int tid = (int)threadIdx.x, phase_once_ = 1; phase_once_; phase_once_ = 0, __syncthreads())
#define SNERF_PNG_SYNC() __syncthreads()
#define SNERF_PNG_ADD(p, v) atomicAdd((p), (v))
#define SNERF_PNG_OR(p, v) atomicOr((p), (v))
#define SNERF_PNG_MAX(p, v) atomicMax((p), (v))
#else
#define SNERF_PNG_FN inline
#define SNERF_PNG_PHASE for (int tid = 0; tid < snerf::png::kThreads; ++tid)
#define SNERF_PNG_SYNC() ((void)0)
#define SNERF_PNG_ADD(p, v) (*(p) += (v))
#define SNERF_PNG_OR(p, v) (*(p) |= (v))
#define SNERF_PNG_MAX(p, v) (*(p) = *(p) < (v) ? (v) : *(p))
#endif

namespace snerf {
namespace png {

constexpr int kThreads = 256;
constexpr int kStrip = 32768;                     // SNERF_PNG_STRIP_BYTES
constexpr int kChunk = kStrip / kThreads;         // consecutive strip bytes owned by one thread
constexpr int kChunkStride = kChunk + 4;          // their stride in LDS: 33 dwords, so that a wave's byte reads at one chunk offset hit 32 banks
constexpr int kSlot = kStrip + 32;                // bytes a coded strip has in the workspace: <= kStrip + 5, written 16 at a time
constexpr int kBitWords = kStrip / 4 + 8;         // the bit buffer, in 32-bit words
constexpr int kLitLen = 286, kEndOfBlock = 256, kLenLimit = 15, kCodeLenSyms = 19, kCodeLenLimit = 7;
constexpr int kMaxSeq = 320;                      // >= 286 + 1 entries of the code-length sequence
constexpr uint32_t kAdler = 65521;

struct StripShared {
    alignas(16) uint32_t bits[kBitWords];
    alignas(16) uint8_t strip[kThreads * kChunkStride];
    uint32_t freq[kLitLen + 2];
    uint32_t weight[2 * (kLitLen + 2)];           // leaves in ascending order, then the internal nodes in creation order
    uint16_t parent[2 * (kLitLen + 2)];
    uint16_t order[kLitLen + 2];                  // leaf -> symbol
    uint16_t code[kLitLen + 2];                   // bit-reversed: as they go into the LSB-first stream
    uint8_t len[kLitLen + 2];
    uint32_t cl_freq[kCodeLenSyms];
    uint16_t cl_code[kCodeLenSyms];
    uint8_t cl_len[kCodeLenSyms];
    uint8_t seq_sym[kMaxSeq], seq_extra[kMaxSeq];
    uint32_t scan[kThreads], scan2[kThreads];     // per-thread values of the block sums
    int last_head[kThreads], first_head[kThreads];    // per chunk: its last / first run start, or -1 / kNone
    int run_start[kThreads], run_end[kThreads];       // per chunk: the start of the run its first byte is in; the first run start after it
    uint32_t bit_offset[kThreads];
    uint32_t bl_count[16], next_code[16];
    int used, deepest, has_match, hlit, seq_count;
    uint32_t header_bits, token_bits, s1, s2;
};

struct FilterShared {
    unsigned long long sums[5][kThreads];
    unsigned long long total[5];
    int type;
};

struct ScanShared {
    unsigned long long sizes[kThreads];
    unsigned long long carry;
};

constexpr int kNone = 0x7fffffff;

SNERF_PNG_FN int strip_at(int p) { return p + (p >> 7) * (kChunkStride - kChunk); }
static_assert(kChunk == 128, "strip_at shifts by log2(kChunk)");

// ------------------------------------------------------------------------------------------------------------ filter
SNERF_PNG_FN int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// filtered byte of type t at x: cur the raw row, up the raw row above (NULL: zeros), bpp bytes per pixel
SNERF_PNG_FN uint8_t filtered(int t, const uint8_t* cur, const uint8_t* up, int x, int bpp) {
    const int v = cur[x];
    const int a = x >= bpp ? cur[x - bpp] : 0;
    const int b = up ? up[x] : 0;
    const int c = (up && x >= bpp) ? up[x - bpp] : 0;
    const int predicted = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? ((a + b) >> 1) : paeth(a, b, c);
    return (uint8_t)(v - predicted);
}

// One row of `row_bytes` = width * channels raw bytes -> out[0] = its type, out[1..] = the filtered row.
SNERF_PNG_FN void filter_row(FilterShared& sh, const uint8_t* cur, const uint8_t* up, int row_bytes, int bpp, int mode, uint8_t* out) {
    if (mode < 0) {
        SNERF_PNG_PHASE {
            unsigned long long sum[5] = {0, 0, 0, 0, 0};
            for (int x = tid; x < row_bytes; x += kThreads) {
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    const int v = filtered(t, cur, up, x, bpp);
                    sum[t] += (unsigned)(v < 128 ? v : 256 - v);
                }
            }
#pragma unroll
            for (int t = 0; t < 5; ++t) sh.sums[t][tid] = sum[t];
        }
        SNERF_PNG_PHASE {
            if (tid < 5) {
                unsigned long long total = 0;
                for (int i = 0; i < kThreads; ++i) total += sh.sums[tid][i];
                sh.total[tid] = total;
            }
        }
        SNERF_PNG_PHASE {
            if (tid == 0) {
                int best = 0;
                for (int t = 1; t < 5; ++t)
                    if (sh.total[t] < sh.total[best]) best = t;       // a tie keeps the lowest type
                sh.type = best;
            }
        }
    }
    const int type = mode < 0 ? sh.type : mode;
    SNERF_PNG_PHASE {
        if (tid == 0) out[0] = (uint8_t)type;
        for (int x = tid; x < row_bytes; x += kThreads) out[1 + x] = filtered(type, cur, up, x, bpp);
    }
}

// ------------------------------------------------------------------------------------------------------------ tokens
// length 3..258 -> its literal/length symbol, the number of extra bits and their value (RFC 1951 3.2.5)
SNERF_PNG_FN void length_symbol(int length, int& symbol, int& extra_bits, int& extra) {
    const int l = length - 3;
    if (length == 258) {
        symbol = 285, extra_bits = 0, extra = 0;
    } else if (l < 8) {
        symbol = 257 + l, extra_bits = 0, extra = 0;
    } else {
        extra_bits = (31 - __builtin_clz((unsigned)l)) - 2;
        symbol = 261 + 4 * extra_bits + ((l >> extra_bits) & 3);
        extra = l & ((1 << extra_bits) - 1);
    }
}

// The tokens that START in thread tid's chunk of a strip of `length` bytes, in order: f.literal(byte) / f.match(length).
template <class F>
SNERF_PNG_FN void walk_tokens(const StripShared& sh, int tid, int length, F& f) {
    const int base = tid * kChunk;
    if (base >= length) return;
    const int end = base + kChunk < length ? base + kChunk : length;
    int p = base, q = sh.run_start[tid];
    while (p < end) {
        // the run [q, e) that p is in
        const int byte = sh.strip[strip_at(p)];
        int e = p + 1;
        while (e < end && sh.strip[strip_at(e)] == byte) ++e;
        if (e == end) e = sh.run_end[tid];
        const int segment_end = e < end ? e : end;
        const int repeats = e - q - 1;                 // bytes of the run after its first: coded as matches of up to 258
        int x = p;
        while (x < segment_end) {
            if (x == q) {
                f.literal(byte);
                ++x;
                continue;
            }
            const int j = x - q - 1, piece = j / 258, within = j - piece * 258;
            const int left = repeats - piece * 258, piece_length = left < 258 ? left : 258;
            if (piece_length < 3) {
                f.literal(byte);
                ++x;
            } else {
                if (within == 0) f.match(piece_length);
                x = q + 1 + piece * 258 + piece_length;      // the next piece (or the next run)
            }
        }
        p = segment_end;
        q = p;
    }
}

struct CountSymbols {
    StripShared& sh;
    SNERF_PNG_FN void literal(int byte) { SNERF_PNG_ADD(&sh.freq[byte], 1u); }
    SNERF_PNG_FN void match(int length) {
        int symbol, extra_bits, extra;
        length_symbol(length, symbol, extra_bits, extra);
        SNERF_PNG_ADD(&sh.freq[symbol], 1u);
        sh.has_match = 1;                              // (every writer writes 1)
    }
};

struct CountBits {
    const StripShared& sh;
    uint32_t bits;
    SNERF_PNG_FN void literal(int byte) { bits += sh.len[byte]; }
    SNERF_PNG_FN void match(int length) {
        int symbol, extra_bits, extra;
        length_symbol(length, symbol, extra_bits, extra);
        bits += sh.len[symbol] + extra_bits + 1;       // + the one-bit distance code
    }
};

// OR `count` <= 32 bits of `value` into the bit buffer at bit `at` (LSB first)
SNERF_PNG_FN void put_bits(uint32_t* words, uint32_t at, uint32_t value, int count) {
    if (count == 0) return;
    const unsigned long long shifted = (unsigned long long)value << (at & 31);
    SNERF_PNG_OR(&words[at >> 5], (uint32_t)shifted);
    const uint32_t high = (uint32_t)(shifted >> 32);
    if (high) SNERF_PNG_OR(&words[(at >> 5) + 1], high);
}

struct EmitTokens {
    StripShared& sh;
    uint32_t at;
    SNERF_PNG_FN void literal(int byte) {
        put_bits(sh.bits, at, sh.code[byte], sh.len[byte]);
        at += sh.len[byte];
    }
    SNERF_PNG_FN void match(int length) {
        int symbol, extra_bits, extra;
        length_symbol(length, symbol, extra_bits, extra);
        const int n = sh.len[symbol];
        put_bits(sh.bits, at, (uint32_t)sh.code[symbol] | ((uint32_t)extra << n), n + extra_bits + 1);     // distance code: one 0 bit
        at += n + extra_bits + 1;
    }
};

// ------------------------------------------------------------------------------------------------------------ codes
// Code lengths <= limit of a Huffman code of freq[0..n): len[i] = 0 where freq[i] = 0.  While the code is deeper than `limit`,
// every count c becomes (c + 1) / 2 and the code is built again (equal counts give depth <= ceil(log2 n)).  Changes freq.
// A single used symbol gets length 1.
SNERF_PNG_FN void build_lengths(StripShared& sh, uint32_t* freq, int n, int limit, uint8_t* len) {
    for (;;) {
        SNERF_PNG_PHASE {
            if (tid == 0) sh.used = 0, sh.deepest = 0;
        }
        SNERF_PNG_PHASE {      // leaves in ascending (count, symbol) order
            for (int i = tid; i < n; i += kThreads) {
                const uint32_t f = freq[i];
                len[i] = 0;
                if (f == 0) continue;
                int rank = 0;
                for (int j = 0; j < n; ++j) {
                    const uint32_t g = freq[j];
                    rank += (g != 0 && (g < f || (g == f && j < i))) ? 1 : 0;
                }
                sh.weight[rank] = f;
                sh.order[rank] = (uint16_t)i;
                SNERF_PNG_MAX(&sh.used, rank + 1);
            }
        }
        const int used = sh.used;
        SNERF_PNG_PHASE {      // the tree, by the two-queue merge: internal node c's children have smaller indices
            if (tid == 0) {
                int leaf = 0, node = used, next = used;
                while (next < 2 * used - 1) {
                    int picked[2];
                    for (int k = 0; k < 2; ++k) {
                        if (leaf < used && (node >= next || sh.weight[leaf] <= sh.weight[node])) picked[k] = leaf++;
                        else picked[k] = node++;
                    }
                    sh.weight[next] = sh.weight[picked[0]] + sh.weight[picked[1]];
                    sh.parent[picked[0]] = sh.parent[picked[1]] = (uint16_t)next;
                    ++next;
                }
            }
        }
        SNERF_PNG_PHASE {
            for (int i = tid; i < used; i += kThreads) {
                int depth = 0;
                for (int k = i; k != 2 * used - 2; k = sh.parent[k]) ++depth;
                if (used == 1) depth = 1;
                len[sh.order[i]] = (uint8_t)(depth < 255 ? depth : 255);
                SNERF_PNG_MAX(&sh.deepest, depth);
            }
        }
        const int deepest = sh.deepest;
        SNERF_PNG_SYNC();      // (everyone has read `used` and `deepest` before anyone clears them again)
        if (deepest <= limit) return;
        SNERF_PNG_PHASE {
            for (int i = tid; i < n; i += kThreads)
                if (freq[i]) freq[i] = (freq[i] + 1) >> 1;
        }
    }
}

SNERF_PNG_FN uint32_t reverse_bits(uint32_t v, int count) {
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
    return v >> (16 - count);
}

// The canonical code of the lengths (RFC 1951 3.2.2), bit-reversed.
SNERF_PNG_FN void assign_codes(StripShared& sh, const uint8_t* len, int n, uint16_t* code) {
    SNERF_PNG_PHASE {
        if (tid < 16) sh.bl_count[tid] = 0;
    }
    SNERF_PNG_PHASE {
        for (int i = tid; i < n; i += kThreads)
            if (len[i]) SNERF_PNG_ADD(&sh.bl_count[len[i]], 1u);
    }
    SNERF_PNG_PHASE {
        if (tid == 0) {
            uint32_t next = 0;
            sh.next_code[0] = 0;
            for (int b = 1; b < 16; ++b) {
                next = (next + (b > 1 ? sh.bl_count[b - 1] : 0u)) << 1;
                sh.next_code[b] = next;
            }
        }
    }
    SNERF_PNG_PHASE {
        for (int i = tid; i < n; i += kThreads) {
            const int l = len[i];
            if (l == 0) {
                code[i] = 0;
                continue;
            }
            uint32_t earlier = 0;
            for (int j = 0; j < i; ++j) earlier += len[j] == l ? 1u : 0u;
            code[i] = (uint16_t)reverse_bits(sh.next_code[l] + earlier, l);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ a strip
SNERF_PNG_FN void load16(const uint8_t* from, uint32_t (&words)[4]) {
#if defined(__HIPCC__)
    const uint4 v = *reinterpret_cast<const uint4*>(from);
    words[0] = v.x, words[1] = v.y, words[2] = v.z, words[3] = v.w;
#else
    memcpy(words, from, 16);
#endif
}

SNERF_PNG_FN void store16(uint8_t* to, const uint32_t* words) {
#if defined(__HIPCC__)
    *reinterpret_cast<uint4*>(to) = make_uint4(words[0], words[1], words[2], words[3]);
#else
    memcpy(to, words, 16);
#endif
}

// One strip: `source` (16-byte aligned; readable up to the next multiple of 16 past `length`) holds its 1 <= length <= kStrip
// filtered bytes.  Writes the strip's deflate block(s) to `slot` (16-byte aligned, kSlot bytes), their byte count to *size and the
// strip's Adler sums (s1, s2 from a zero state, mod 65521) to adler[0..1].
SNERF_PNG_FN void encode_strip(StripShared& sh, const uint8_t* source, int length, bool final, uint8_t* slot, int* size, uint32_t* adler) {
    SNERF_PNG_PHASE {
        for (int i = tid; i < kBitWords; i += kThreads) sh.bits[i] = 0;
        for (int i = tid; i < kLitLen + 2; i += kThreads) sh.freq[i] = 0;
        if (tid == 0) sh.has_match = 0;
        for (int v = tid; v * 16 < length; v += kThreads) {
            uint32_t words[4];
            load16(source + v * 16, words);
            uint8_t* to = &sh.strip[strip_at(v * 16)];       // (16 bytes never straddle a chunk, and strip_at keeps 4-byte alignment)
#pragma unroll
            for (int k = 0; k < 4; ++k) *reinterpret_cast<uint32_t*>(to + 4 * k) = words[k];
        }
    }
    SNERF_PNG_PHASE {      // per chunk: Adler partial sums, first and last run start
        const int base = tid * kChunk;
        const int end = base + kChunk < length ? base + kChunk : length;
        uint32_t s1 = 0, s2 = 0;       // s2 <= 128 * 32768 * 255 < 2^31
        int first = kNone, last = -1;
        for (int p = base; p < end; ++p) {
            const uint32_t byte = sh.strip[strip_at(p)];
            s1 += byte;
            s2 += (uint32_t)(length - p) * byte;
            if (p == 0 || sh.strip[strip_at(p - 1)] != byte) {
                if (first == kNone) first = p;
                last = p;
            }
        }
        sh.scan[tid] = s1;
        sh.scan2[tid] = s2 % kAdler;
        sh.first_head[tid] = first;
        sh.last_head[tid] = last;
    }
    SNERF_PNG_PHASE {      // what a chunk needs to know of its neighbours (a flat strip makes these walks long, its token walk short)
        int start = sh.first_head[tid] == tid * kChunk ? tid * kChunk : -1;
        for (int t = tid - 1; t >= 0 && start < 0; --t) start = sh.last_head[t];
        sh.run_start[tid] = start < 0 ? 0 : start;
        int next = kNone;
        for (int t = tid + 1; t < kThreads && next == kNone; ++t) next = sh.first_head[t];
        sh.run_end[tid] = next == kNone ? length : next;
        if (tid == 0) {
            uint32_t s1 = 0, s2 = 0;
            for (int t = 0; t < kThreads; ++t) s1 += sh.scan[t], s2 += sh.scan2[t];
            sh.s1 = s1 % kAdler, sh.s2 = s2 % kAdler;
        }
    }
    SNERF_PNG_PHASE {
        CountSymbols count{sh};
        walk_tokens(sh, tid, length, count);
        if (tid == 0) SNERF_PNG_ADD(&sh.freq[kEndOfBlock], 1u);
    }
    build_lengths(sh, sh.freq, kLitLen, kLenLimit, sh.len);
    assign_codes(sh, sh.len, kLitLen, sh.code);
    const int distance_len = sh.has_match ? 1 : 0;
    SNERF_PNG_PHASE {      // the code lengths of the literal/length symbols and of the one distance symbol as code-length symbols
        if (tid == 0) {
            int hlit = kLitLen;
            while (hlit > 257 && sh.len[hlit - 1] == 0) --hlit;
            sh.hlit = hlit;
            for (int s = 0; s < kCodeLenSyms; ++s) sh.cl_freq[s] = 0;
            const int n = hlit + 1;
            int count = 0, i = 0;
            while (i < n) {
                const int value = i < hlit ? sh.len[i] : distance_len;
                int run = 1;
                while (i + run < n && (i + run < hlit ? sh.len[i + run] : distance_len) == value) ++run;
                i += run;
                if (value == 0) {
                    while (run >= 11) {
                        const int take = run < 138 ? run : 138;
                        sh.seq_sym[count] = 18, sh.seq_extra[count++] = (uint8_t)(take - 11);
                        run -= take;
                    }
                    if (run >= 3) {
                        sh.seq_sym[count] = 17, sh.seq_extra[count++] = (uint8_t)(run - 3);
                        run = 0;
                    }
                } else {
                    sh.seq_sym[count] = (uint8_t)value, sh.seq_extra[count++] = 0;
                    --run;
                    while (run >= 3) {
                        const int take = run < 6 ? run : 6;
                        sh.seq_sym[count] = 16, sh.seq_extra[count++] = (uint8_t)(take - 3);
                        run -= take;
                    }
                }
                for (; run > 0; --run) sh.seq_sym[count] = (uint8_t)value, sh.seq_extra[count++] = 0;
            }
            sh.seq_count = count;
            for (int k = 0; k < count; ++k) sh.cl_freq[sh.seq_sym[k]] += 1;
        }
    }
    build_lengths(sh, sh.cl_freq, kCodeLenSyms, kCodeLenLimit, sh.cl_len);
    assign_codes(sh, sh.cl_len, kCodeLenSyms, sh.cl_code);
    SNERF_PNG_PHASE {      // thread 0: the block header; everyone: the bits of its tokens
        if (tid == 0) {
            const int order[kCodeLenSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint32_t at = 0;
            put_bits(sh.bits, at, final ? 1u : 0u, 1), at += 1;
            put_bits(sh.bits, at, 2u, 2), at += 2;                                  // BTYPE = 10
            put_bits(sh.bits, at, (uint32_t)(sh.hlit - 257), 5), at += 5;
            put_bits(sh.bits, at, 0u, 5), at += 5;                                  // HDIST: one distance code
            int hclen = kCodeLenSyms;
            while (hclen > 4 && sh.cl_len[order[hclen - 1]] == 0) --hclen;
            put_bits(sh.bits, at, (uint32_t)(hclen - 4), 4), at += 4;
            for (int k = 0; k < hclen; ++k) put_bits(sh.bits, at, sh.cl_len[order[k]], 3), at += 3;
            for (int k = 0; k < sh.seq_count; ++k) {
                const int s = sh.seq_sym[k];
                put_bits(sh.bits, at, sh.cl_code[s], sh.cl_len[s]), at += sh.cl_len[s];
                const int extra_bits = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
                put_bits(sh.bits, at, sh.seq_extra[k], extra_bits), at += extra_bits;
            }
            sh.header_bits = at;
        }
        CountBits count{sh, 0};
        walk_tokens(sh, tid, length, count);
        sh.scan[tid] = count.bits;
    }
    SNERF_PNG_PHASE {
        uint32_t before = 0;
        for (int t = 0; t < tid; ++t) before += sh.scan[t];
        sh.bit_offset[tid] = before;
        if (tid == kThreads - 1) sh.token_bits = before + sh.scan[tid];
    }
    // coded or stored: header + tokens + end of block; a strip that is not the last ends on a byte boundary
    const unsigned long long total_bits = (unsigned long long)sh.header_bits + sh.token_bits + sh.len[kEndOfBlock];
    const bool aligned = (total_bits & 7) == 0;
    const unsigned long long coded_bytes = (final || aligned) ? (total_bits + 7) / 8 : (total_bits + 3 + 7) / 8 + 4;
    const int stored_bytes = length + 5;
    if (coded_bytes < (unsigned long long)stored_bytes) {
        SNERF_PNG_PHASE {
            EmitTokens emit{sh, sh.header_bits + sh.bit_offset[tid]};
            walk_tokens(sh, tid, length, emit);
            if (tid == 0) {
                put_bits(sh.bits, sh.header_bits + sh.token_bits, sh.code[kEndOfBlock], sh.len[kEndOfBlock]);
                if (!final && !aligned) put_bits(sh.bits, (uint32_t)(coded_bytes - 2) * 8, 0xffffu, 16);     // 000, padding, 00 00 FF FF
            }
        }
        SNERF_PNG_PHASE {
            for (int v = tid; v * 16 < (int)coded_bytes; v += kThreads) store16(slot + v * 16, &sh.bits[v * 4]);
            if (tid == 0) *size = (int)coded_bytes;
        }
    } else {
        SNERF_PNG_PHASE {
            if (tid == 0) {
                slot[0] = final ? 1 : 0;
                slot[1] = (uint8_t)(length & 255), slot[2] = (uint8_t)(length >> 8);
                slot[3] = (uint8_t)(~length & 255), slot[4] = (uint8_t)((~length >> 8) & 255);
                *size = stored_bytes;
            }
            for (int p = tid; p < length; p += kThreads) slot[5 + p] = sh.strip[strip_at(p)];
        }
    }
    SNERF_PNG_PHASE {
        if (tid == 0) adler[0] = sh.s1, adler[1] = sh.s2;
    }
}

// ------------------------------------------------------------------------------------------------------------ a frame's stream
// Offsets of a frame's `strips` coded strips in its stream (after the 2-byte zlib header), the header, the Adler-32 of its `raw`
// filtered bytes and the stream's length.
SNERF_PNG_FN void scan_frame(ScanShared& sh, const int* sizes, const uint32_t* adler, int strips, int raw, long long* offsets,
                             uint8_t* stream, long long* stream_bytes) {
    SNERF_PNG_PHASE {
        if (tid == 0) sh.carry = 2;
    }
    for (int first = 0; first < strips; first += kThreads) {
        const unsigned long long carry = sh.carry;
        SNERF_PNG_PHASE { sh.sizes[tid] = first + tid < strips ? (unsigned long long)sizes[first + tid] : 0ull; }
        SNERF_PNG_PHASE {
            unsigned long long at = carry;
            for (int t = 0; t < tid; ++t) at += sh.sizes[t];
            if (first + tid < strips) offsets[first + tid] = (long long)at;
            if (tid == kThreads - 1) sh.carry = at + sh.sizes[tid];
        }
    }
    SNERF_PNG_PHASE {
        if (tid == 0) {
            unsigned long long a = 1, b = 0;
            for (int s = 0; s < strips; ++s) {
                const int length = raw - s * kStrip < kStrip ? raw - s * kStrip : kStrip;
                b = (b + (unsigned long long)length * a + adler[2 * s + 1]) % kAdler;
                a = (a + adler[2 * s]) % kAdler;
            }
            const unsigned long long end = sh.carry;
            stream[0] = 0x78, stream[1] = 0x9c;
            stream[end] = (uint8_t)(b >> 8), stream[end + 1] = (uint8_t)b, stream[end + 2] = (uint8_t)(a >> 8), stream[end + 3] = (uint8_t)a;
            *stream_bytes = (long long)(end + 4);
        }
    }
}

SNERF_PNG_FN void pack_strip(const uint8_t* slot, int size, uint8_t* to) {
    SNERF_PNG_PHASE {
        for (int i = tid; i < size; i += kThreads) to[i] = slot[i];
    }
}

}  // namespace png
}  // namespace snerf
