// The layered MLP path (mlp_generic.hip) on bf16 operands: hip_precision 'bf16' and 'bf16s8' for every shape the fused kernels are
// not built for.  The same layer walk as the fp32 path (mlp_generic_walk.h); this file is the bf16 operand format it is instantiated
// with, with the mode semantics of the fused bf16 kernels: fp32 master weights rounded to bf16 as they are staged (the
// packed buffer is the fp32 path's, unchanged), encodings, hidden activations and layer gradients dZ held as bf16, fp32
// accumulation, and the heads, sigma, rgb, the density noise, the bias sums and the split-K partial sums in fp32.  'bf16s8' is
// 'bf16' here: the fp8 saved trunk exists for the fused 256-wide kernels only.
//
// Activation matrix: one row of bf16 per sample, the fp32 path's blocks in the same order but each starting at a multiple of EIGHT
// elements (16 bytes: the GEMM stages 8 bf16 per load), followed by an fp32 [N][8] block for the two heads' outputs (pts_output in
// columns 0-3, views_output in 4-7).  Both fit in the generic_saved_floats() the fp32 path reports (checked per call).  The backward
// workspace holds its dZ ping-pong as bf16 with a row stride of the widest layer rounded up to eight; the rest as in the fp32 path.
//
// GEMM: C(m,n) = sum_k A(m,k) B(k,n) on v_mfma_f32_32x32x16_bf16, 64 x 64 or 128 x 128 output tile per 256-thread workgroup (2 x 2
// waves), K staged through LDS 64 at a time with the next stage's global loads in flight.  Every operand of the path is contiguous
// along k (forward: activations and W; input gradient: dZ) or along its rows m resp. n (weight gradient: dZ^T and X; input
// gradient: W[:, cols]).  The first kind is staged as a [row][k] image and read with ds_read_b128, the second as a [k][row] image
// and read with ds_read_b64_tr_b16 (the hardware transposes 4 k x 16 rows per 16-lane group).  Either is filled 8 elements per
// thread and group: one 16-byte load (bf16) or two (fp32, rounded to bf16 with v_cvt_pk_bf16_f32 as they are stored) where
// strides and addresses allow it, element by element otherwise (the ragged 63-, 575- and 539-wide products of the fp32 weights).
#include <algorithm>

#include "mlp_device.h"
#include "mlp_generic.h"
#include "mlp_generic_kernels.h"
#include "mlp_generic_walk.h"

namespace {

typedef unsigned short bf16_t;                                    // bf16 bits in memory
typedef __bf16 gbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gbf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int gu32x4 __attribute__((ext_vector_type(4)));
typedef short gs16x4 __attribute__((ext_vector_type(4)));
typedef short gs16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float bf16_value(bf16_t b) { return __uint_as_float((unsigned)b << 16); }
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {      // round to nearest even: v_cvt_pk_bf16_f32
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, gbf16x2));
}

struct GemmBf16Args {
    const void* A; long long a_rs, a_cs;       // element type and layout are template arguments of the kernel
    const void* B; long long b_rs, b_cs;
    void* C; long long c_rs;                   // (column stride 1)
    const float* bias;                         // per column n, or NULL
    const bf16_t* mask; long long mask_rs;     // C(m,n) *= (mask[m * mask_rs + n] > 0), or NULL (ReLU gate of the backward)
    int M, N, K;
    int relu, accumulate;
    long long k_chunk;                         // split-K: blockIdx.z owns k in [z * k_chunk, min(K, (z+1) * k_chunk)) and writes
    long long split_stride;                    // C + z * split_stride (a partial-sum buffer); 0 = no split
    int a_vec, b_vec;                          // 16-byte global loads allowed for A / B (launch16 decides)
};

constexpr int kBK16 = 64;                      // k per stage
constexpr int kKRow = kBK16 + 8;               // bf16 per row of a [row][k] image: 144-byte rows, ds_read_b128 conflict-free
constexpr int kTrPad = 32;                     // [k][row] image rows of TILE + 32 bf16 (320 / 192 bytes): tr reads conflict-free

// One operand tile (TILE rows of m resp. n  x  kBK16 of k) from memory into LDS as bf16.  `st` = stride (elements) between
// neighbouring rows, `sk` = between neighbouring k.  LAYOUT 0: sk == 1, image [TILE][kKRow]; LAYOUT 1: st == 1, image
// [kBK16][TILE + kTrPad].  A thread owns TILE / 32 groups of 8 elements contiguous in memory (and in LDS).
template <int TILE, int LAYOUT, typename T>
struct Stage16 {
    static constexpr int kGroups = TILE / 32;
    static constexpr int kTrRow = TILE + kTrPad;
    static constexpr int kImage = LAYOUT == 0 ? TILE * kKRow : kBK16 * kTrRow;     // bf16 per stage buffer
    static constexpr int kStepK = 256 / (TILE / 8);                                 // LAYOUT 1: k rows per pass of the 256 threads
    const T* tile;               // element (row 0, k 0) of the tile
    long long st, sk;
    int left;                    // rows of the tile inside the matrix
    int t0, k0;                  // this thread's first group: row, k
    T r[kGroups][8];
    unsigned inside;             // bit 8 e + j: element j of group e of the stage in flight lies inside the matrix

    __device__ __forceinline__ int row_of(int e) const { return LAYOUT == 0 ? t0 + 32 * e : t0; }
    __device__ __forceinline__ int k_of(int e) const { return LAYOUT == 0 ? k0 : k0 + kStepK * e; }
    __device__ __forceinline__ void init(const T* first, long long st_, long long sk_, int left_, int tid) {
        tile = first; st = st_; sk = sk_; left = left_;
        if constexpr (LAYOUT == 0) { t0 = tid >> 3; k0 = (tid & 7) * 8; }
        else { t0 = (tid % (TILE / 8)) * 8; k0 = tid / (TILE / 8); }
    }
    // An element outside the matrix reads the stage's first element (always inside) and is replaced by zero WHEN IT IS STORED, after
    // this stage's MFMAs.  vec: a group is one (bf16) or two (fp32) 16-byte loads; a group partly inside reads past the matrix's
    // edge only where launch16 allowed it (the padded rows of this path's bf16 buffers).
    __device__ __forceinline__ void load(long long k_first, int k_left, bool vec) {
        const T* stage = tile + k_first * sk;
        inside = 0;
#pragma unroll
        for (int e = 0; e < kGroups; ++e) {
            const int t = row_of(e), k = k_of(e);
            unsigned in8 = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool in = LAYOUT == 0 ? (t < left && k + j < k_left) : (t + j < left && k < k_left);
                in8 |= in ? 1u << j : 0u;
            }
            inside |= in8 << (8 * e);
            const unsigned base = in8 ? (unsigned)((long long)t * st + (long long)k * sk) : 0u;
            if (vec) {
                if constexpr (sizeof(T) == 2) {
                    const gs16x8 v = *reinterpret_cast<const gs16x8*>(stage + base);
#pragma unroll
                    for (int j = 0; j < 8; ++j) r[e][j] = (T)v[j];
                } else {
                    const f32x4 lo = *reinterpret_cast<const f32x4*>(stage + base);
                    const f32x4 hi = *reinterpret_cast<const f32x4*>(stage + base + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { r[e][j] = lo[j]; r[e][4 + j] = hi[j]; }
                }
            } else {
                const long long step = LAYOUT == 0 ? sk : st;
#pragma unroll
                for (int j = 0; j < 8; ++j) r[e][j] = stage[(in8 >> j) & 1u ? base + (unsigned)(j * step) : 0u];
            }
        }
    }
    __device__ __forceinline__ void store(bf16_t* buffer) const {
#pragma unroll
        for (int e = 0; e < kGroups; ++e) {
            unsigned w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool in_lo = (inside >> (8 * e + 2 * q)) & 1u, in_hi = (inside >> (8 * e + 2 * q + 1)) & 1u;
                if constexpr (sizeof(T) == 2) {
                    w[q] = (in_lo ? (unsigned)r[e][2 * q] : 0u) | ((in_hi ? (unsigned)r[e][2 * q + 1] : 0u) << 16);
                } else {
                    w[q] = pack_bf16(in_lo ? r[e][2 * q] : 0.0f, in_hi ? r[e][2 * q + 1] : 0.0f);
                }
            }
            const gu32x4 v = {w[0], w[1], w[2], w[3]};
            const int at = LAYOUT == 0 ? row_of(e) * kKRow + k_of(e) : k_of(e) * kTrRow + row_of(e);
            *reinterpret_cast<gu32x4*>(buffer + at) = v;
        }
    }
};

// MFMA operand of the 32 rows starting at row0, k-step s of the stage: lane (r = lane & 31, h = lane >> 5) gets k = 16 s + 8 h + j
// of row row0 + r in element j.  (LAYOUT 1: every lane of the wave takes part -- ds_read_b64_tr_b16 needs EXEC all ones; nothing
// around these reads is divergent.)
template <int TILE, int LAYOUT>
__device__ __forceinline__ gbf16x8 fragment(const bf16_t* buffer, int row0, int s, int lane) {
    if constexpr (LAYOUT == 0) {
        return __builtin_bit_cast(gbf16x8, *reinterpret_cast<const gu32x4*>(buffer + (row0 + (lane & 31)) * kKRow + 16 * s + 8 * (lane >> 5)));
    } else {
        // lane 4q + p of a 16-lane group g supplies row (k) q, columns 4p .. 4p + 3 of its 4 x 16 block; lane i of the group
        // receives column i: the group covers rows row0 + 16 (g & 1) + (0..15), k = 16 s + 8 (g >> 1) + (0..3), then + 4
        constexpr int kTrRow = TILE + kTrPad;
        const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
        const bf16_t* a = buffer + (16 * s + 8 * (g >> 1) + q) * kTrRow + row0 + 16 * (g & 1) + 4 * p;
        const gs16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) gs16x4*)(a));
        const gs16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) gs16x4*)(a + 4 * kTrRow));
        const gs16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(gbf16x8, both);
    }
}

template <typename TC> __device__ __forceinline__ float load_c(const TC* p);
template <> __device__ __forceinline__ float load_c<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float load_c<bf16_t>(const bf16_t* p) { return bf16_value(*p); }

// Accumulators -> C (+ bias, + C, ReLU, gate) in fp32, stored as TC.  D layout: lane (i = column, h), register r -> row
// (r & 3) + 8 (r >> 2) + 4 h of the 32 x 32 tile.  Whole tiles read what they add to and the gate in one batch (as the fp32 path).
template <int TM, int TN, typename TC>
__device__ __forceinline__ void write_tile16(const f32x16 (&acc)[TM][TN], const GemmBf16Args& g, TC* C, int m0, int n0, int wm, int wn,
                                             int i, int h) {
    const bool whole = m0 + 64 * TM <= g.M && n0 + 64 * TN <= g.N;
    if (whole) {
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const long long n = n0 + wn + 32 * tn + i;
            const float bias = g.bias ? g.bias[n] : 0.0f;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) {
                const long long m_first = m0 + wm + 32 * tm + 4 * h;
                TC* const dst = C + m_first * g.c_rs + n;
                const bf16_t* const gate = g.mask ? g.mask + m_first * g.mask_rs + n : nullptr;
                float old[16], open[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long dm = (r & 3) + 8 * (r >> 2);
                    old[r] = g.accumulate ? load_c<TC>(dst + dm * g.c_rs) : 0.0f;
                    open[r] = gate ? bf16_value(gate[dm * g.mask_rs]) : 1.0f;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long dm = (r & 3) + 8 * (r >> 2);
                    float v = acc[tm][tn][r] + bias;
                    if (g.accumulate) v += old[r];
                    if (g.relu) v = fmaxf(v, 0.0f);
                    if (g.mask) v = open[r] > 0.0f ? v : 0.0f;
                    dst[dm * g.c_rs] = store_as<TC>(v);
                }
            }
        }
        return;
    }
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const long long n = n0 + wn + 32 * tn + i;
        if (n >= g.N) continue;
        const float bias = g.bias ? g.bias[n] : 0.0f;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long m = m0 + wm + 32 * tm + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m >= g.M) continue;
                float v = acc[tm][tn][r] + bias;
                TC* dst = C + m * g.c_rs + n;
                if (g.accumulate) v += load_c<TC>(dst);
                if (g.relu) v = fmaxf(v, 0.0f);
                if (g.mask) v = bf16_value(g.mask[m * g.mask_rs + n]) > 0.0f ? v : 0.0f;
                *dst = store_as<TC>(v);
            }
    }
}

// BM x BN output tile per 256-thread workgroup = a 2 x 2 grid of waves, each (BM / 2) x (BN / 2) = TM x TN MFMA tiles of 32 x 32.
// LA / LB: Stage16 layouts of A and B; TA / TB: their element types in memory (bf16_t or float); TC: C's.
template <int BM, int BN, int LA, int LB, typename TA, typename TB, typename TC>
__global__ void __launch_bounds__(256, 2) gemm_bf16_kernel(GemmBf16Args g) {
    constexpr int TM = BM / 64, TN = BN / 64;
    using StageA = Stage16<BM, LA, TA>;
    using StageB = Stage16<BN, LB, TB>;
    __shared__ __attribute__((aligned(16))) bf16_t As[2][StageA::kImage];
    __shared__ __attribute__((aligned(16))) bf16_t Bs[2][StageB::kImage];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // tile of this workgroup; XCD-aware order as in the fp32 path's gemm_kernel (a row block's n tiles on one XCD's L2)
    int tile_m = blockIdx.y, tile_n = blockIdx.x;
    if ((gridDim.y & 7u) == 0) {
        const unsigned linear = blockIdx.y * gridDim.x + blockIdx.x, xcd = linear & 7u, idx = linear >> 3;
        tile_m = (int)((idx / gridDim.x) * 8u + xcd);
        tile_n = (int)(idx % gridDim.x);
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const long long k_lo = g.split_stride ? (long long)blockIdx.z * g.k_chunk : 0;
    const long long k_hi = g.split_stride ? (k_lo + g.k_chunk < g.K ? k_lo + g.k_chunk : g.K) : g.K;
    TC* C = static_cast<TC*>(g.C) + (g.split_stride ? (long long)blockIdx.z * g.split_stride : 0);

    StageA sa;
    StageB sb;
    sa.init(static_cast<const TA*>(g.A) + (long long)m0 * g.a_rs, g.a_rs, g.a_cs, g.M - m0, tid);
    sb.init(static_cast<const TB*>(g.B) + (long long)n0 * g.b_cs, g.b_cs, g.b_rs, g.N - n0, tid);
    const bool a_vec = g.a_vec != 0, b_vec = g.b_vec != 0;
    auto load_stage = [&](long long k0) {
        const int k_left = (int)(k_hi - k0 < kBK16 ? k_hi - k0 : kBK16);      // 64 except in the last stage of a ragged K
        sa.load(k0, k_left, a_vec);
        sb.load(k0, k_left, b_vec);
    };

    const int wm = (wave >> 1) * (32 * TM), wn = (wave & 1) * (32 * TN), i = lane & 31, h = lane >> 5;
    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.0f;
    if (k_lo < k_hi) {
        load_stage(k_lo);
        sa.store(As[0]);
        sb.store(Bs[0]);
        __syncthreads();
        int buf = 0;
        for (long long k0 = k_lo; k0 < k_hi; k0 += kBK16) {
            const bool more = k0 + kBK16 < k_hi;
            if (more) load_stage(k0 + kBK16);                    // in flight during this stage's MFMAs
#pragma unroll
            for (int s = 0; s < kBK16 / 16; ++s) {
                gbf16x8 av[TM], bv[TN];
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) av[tm] = fragment<BM, LA>(As[buf], wm + 32 * tm, s, lane);
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) bv[tn] = fragment<BN, LB>(Bs[buf], wn + 32 * tn, s, lane);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[tm], bv[tn], acc[tm][tn], 0, 0, 0);
            }
            if (more) {
                sa.store(As[buf ^ 1]);
                sb.store(Bs[buf ^ 1]);
                __syncthreads();
                buf ^= 1;
            }
        }
    }
    write_tile16<TM, TN, TC>(acc, g, C, m0, n0, wm, wn, i, h);
}

// column sums of bf16 dZ (rows x cols, row stride ld: a multiple of 8, 16-byte aligned; columns up to the next multiple of 8 are
// readable) over a chunk of rows, in fp32: partial[z][col].  A lane owns eight columns (one 16-byte load per row), a wave 512, the
// eight waves of a workgroup take the rows of their chunk in turn, eight rows in flight; a lane adds its rows in order, the waves'
// sums are added in wave order: fixed, whatever the timing.
__global__ void __launch_bounds__(512) colsum8_bf16_kernel(const bf16_t* __restrict__ dz, long long ld, long long rows, int cols,
                                                           long long rows_per_split, float* __restrict__ partial) {
    constexpr int kParts = 8, kAhead = 8;
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * 8;
    const long long lo = (long long)blockIdx.y * rows_per_split, hi = lo + rows_per_split < rows ? lo + rows_per_split : rows;
    float s[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    auto add = [&](const gu32x4& v) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s[2 * q] += __uint_as_float(v[q] << 16);
            s[2 * q + 1] += __uint_as_float(v[q] & 0xffff0000u);
        }
    };
    if (col < cols) {
        const bf16_t* base = dz + col;
        long long r = lo + part;
        for (; r + (long long)(kAhead - 1) * kParts < hi; r += (long long)kAhead * kParts) {
            gu32x4 v[kAhead];
#pragma unroll
            for (int e = 0; e < kAhead; ++e) v[e] = *reinterpret_cast<const gu32x4*>(base + (r + (long long)e * kParts) * ld);
#pragma unroll
            for (int e = 0; e < kAhead; ++e) add(v[e]);
        }
        for (; r < hi; r += kParts) add(*reinterpret_cast<const gu32x4*>(base + r * ld));
    }
    __shared__ float sh[kParts][8][64];
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[part][j][lane] = s[j];
    __syncthreads();
    if (part == 0 && col < cols) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float t = sh[0][j][lane];
#pragma unroll
            for (int q = 1; q < kParts; ++q) t += sh[q][j][lane];
            if (col + j < cols) partial[(long long)blockIdx.y * cols + col + j] = t;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
template <int LA, int LB, typename TA, typename TB, typename TC>
int launch16(const GemmBf16Args& g, int splits, hipStream_t s) {
    if (g.M <= 0 || g.N <= 0) return SNERF_OK;
    int tile = 0;
    const dim3 grid = gemm_grid(g.M, g.N, splits, &tile);
    if (tile == 128) hipLaunchKernelGGL((gemm_bf16_kernel<128, 128, LA, LB, TA, TB, TC>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((gemm_bf16_kernel<64, 64, LA, LB, TA, TB, TC>), grid, dim3(256), 0, s, g);
    return snerf::check_launch("mlp_generic_bf16(gemm)");
}

// May an operand be read 16 bytes at a time?  base: its first element; stride: elements between neighbouring rows (LAYOUT 0) resp.
// k (LAYOUT 1); extent: elements along the contiguous direction (K, or the rows M / N).  bf16 operands are this path's own
// activation rows and dZ buffers: every block starts at a multiple of eight elements and is followed by its row's padding up to the
// next multiple of eight, so a group that crosses the edge stays inside the allocation (the elements past the edge are zeroed).  fp32
// operands (the weights, the head gradients) get no such slack: whole groups only.
bool vec_bf16(const void* base, long long stride) { return aligned16(base) && stride % 8 == 0; }
bool vec_f32(const void* base, long long stride, long long extent) { return aligned16(base) && stride % 4 == 0 && extent % 8 == 0; }
template <typename T> bool vec(const T* base, long long stride, long long extent) {
    return sizeof(T) == 2 ? vec_bf16(base, stride) : vec_f32(base, stride, extent);
}

// The bf16 operand format of the layer walk (row and workspace: top of this file).  A dZ is bf16 (a layer's) or fp32 (a head's): TA.
struct Bf16Operands {
    using Act = bf16_t;
    static constexpr const char* kName = "mlp_generic_bf16";
    static constexpr int kAlign = 8;
    static constexpr bool kHeadsInRow = false;
    static long long ld(long long width) { return (width + 7) / 8 * 8; }
    static long long floats(long long elems) { return (elems + 7) / 8 * 4; }      // whole 16-byte groups

    // Y[rows, out] = act(X[rows, in] . W[out, in]^T + b), X bf16 columns of the activation matrix, Y bf16 columns or the fp32 heads block
    template <typename TC>
    static int linear(const bf16_t* x, long long x_rs, TC* y, long long y_rs, long long rows, int in, int out, const float* w,
                      const float* b, bool relu, hipStream_t s) {
        GemmBf16Args g = {};
        g.A = x; g.a_rs = x_rs; g.a_cs = 1;
        g.B = w; g.b_rs = 1; g.b_cs = in;
        g.C = y; g.c_rs = y_rs;
        g.bias = b; g.M = (int)rows; g.N = out; g.K = in; g.relu = relu ? 1 : 0;
        g.a_vec = vec_bf16(x, x_rs);
        g.b_vec = vec_f32(w, in, in);
        return launch16<0, 0, bf16_t, float, TC>(g, 0, s);
    }
    template <typename TA>
    static int input_grad(const TA* dz, long long dz_ld, int out, const float* w, int w_ld, int cols, bf16_t* dx, long long dx_ld,
                          bool add, const bf16_t* gate, long long gate_rs, long long rows, hipStream_t s) {
        GemmBf16Args g = {};
        g.A = dz; g.a_rs = dz_ld; g.a_cs = 1;
        g.B = w; g.b_rs = w_ld; g.b_cs = 1;
        g.C = dx; g.c_rs = dx_ld;
        g.M = (int)rows; g.N = cols; g.K = out; g.accumulate = add ? 1 : 0;
        g.mask = gate; g.mask_rs = gate_rs;
        g.a_vec = vec(dz, dz_ld, out);
        g.b_vec = vec_f32(w, w_ld, cols);
        return launch16<0, 1, TA, float, bf16_t>(g, 0, s);
    }
    template <typename TA>
    static int wgrad_gemm(const TA* dz, long long dz_ld, int out, const bf16_t* x, long long x_rs, int in, long long total, int splits,
                          long long k_chunk, float* partial, hipStream_t s) {
        GemmBf16Args g = {};
        g.A = dz; g.a_rs = 1; g.a_cs = dz_ld;           // A(m = out feature, k = sample) = dZ[k][m]
        g.B = x; g.b_rs = x_rs; g.b_cs = 1;             // B(k = sample, n = in feature)
        g.C = partial; g.c_rs = in;
        g.M = out; g.N = in; g.K = (int)total; g.k_chunk = k_chunk; g.split_stride = (long long)out * in;
        g.a_vec = vec(dz, dz_ld, out);
        g.b_vec = vec_bf16(x, x_rs);
        return launch16<1, 1, TA, bf16_t, float>(g, splits, s);
    }
    static int colsum(const bf16_t* dz, long long dz_ld, int out, long long total, int bsplits, long long b_chunk, float* bpart,
                      hipStream_t s) {
        if (dz_ld % 8 != 0 || !aligned16(dz)) return snerf::fail(SNERF_E_INVALID, "mlp_backward(layered, bf16): workspace not 16-byte aligned");
        hipLaunchKernelGGL(colsum8_bf16_kernel, dim3((out + 511) / 512, bsplits), dim3(512), 0, s, dz, dz_ld, total, out, b_chunk, bpart);
        return SNERF_OK;
    }
    static int colsum(const float* dz, long long dz_ld, int out, long long total, int bsplits, long long b_chunk, float* bpart, hipStream_t s) {
        hipLaunchKernelGGL(colsum_kernel, dim3((out + 63) / 64, bsplits), dim3(256), 0, s, dz, dz_ld, total, out, b_chunk, bpart);
        return SNERF_OK;
    }
};

}  // namespace

namespace snerf {

int generic_forward_bf16(const GenericPlan& p, const float* packed, const float* origins, const float* dirs, const float* view_dirs,
                         const float* depths, long long num_rays, int num_samples, const float* noise, float* sigma, float* rgb,
                         float* saved_acts, hipStream_t s) {
    return forward_call<Bf16Operands>(p, packed, origins, dirs, view_dirs, depths, num_rays, num_samples, noise, sigma, rgb, saved_acts, s);
}

int generic_backward_bf16(const GenericPlan& p, const float* packed, const float* acts, const float* sigma, const float* rgb,
                          const float* d_sigma, const float* d_rgb, long long total, float* workspace, float* const* grads,
                          int accumulate, hipStream_t s) {
    return backward_walk<Bf16Operands>(p, packed, acts, sigma, rgb, d_sigma, d_rgb, total, workspace, grads, accumulate, s);
}

}  // namespace snerf
