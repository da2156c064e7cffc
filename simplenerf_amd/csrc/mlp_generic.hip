// The layered path of the NeRF MLP for shapes the register-resident fused kernels are not built for: any points_net_width
// (64, 96, 512, ...), any views_net_width, views_net_depth > 1, any depth -- everything MLP.__init__ can build
// (src/models/SimpleNeRF01.py:567-609) except predict_visibility.  Same C ABI, same parameter tensors, same semantics; the
// fused kernels keep every shape they cover (mlp_plan.h build_plan), this file takes the rest so that the reference's config
// keys are honoured instead of refused.
//
// Design.  A 512-wide layer does not fit the register-resident chain (16 accumulator tiles + 16 operand tiles per wave > the
// 512-register file), so activations live in memory here: one row per sample in an [N][row] fp32 matrix
//     [ encoding | view encoding | H_0 ... (the skip layer's input stored as ONE block [encoding | H_4]) ... H_D-1 |
//       views input block [feature | rest of the encoding | view encoding] | HV_0 ... | pts_output | views_output ]
// and every Linear layer is one launch of ONE strided GEMM kernel on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32
// FMA chains, the parity arithmetic): C(m,n) = sum_k A(m,k) B(k,n) with row / column strides for all three matrices, so the
// forward (X . W^T), the input gradient (dZ . W), the weight gradient (dZ^T . X, split over the samples with a fixed-order
// reduction) and the concatenations (column offsets into the row) are the same kernel.  64 x 64 output tile per 256-thread
// workgroup, K staged through LDS 32 at a time with the next stage's global loads in flight.  Bias, ReLU, the ReLU mask of the
// backward and accumulation are epilogue options.
//
// Bound: MFMA fp32 for the wide layers (2 x 4 B x width per sample and layer over HBM against 2 x width^2 FLOP: MFMA-bound from
// width ~100 up), at the efficiency of a plain LDS-tiled GEMM -- a fallback for generality, not the headline path.
// The layer walk -- which layer reads and writes which columns with which parameters, forward and backward -- is written once
// (mlp_generic_walk.h) for two operand formats: this file is the fp32 one (its GEMMs, its row) together with the plan, the entry
// points and their precision gate; mlp_generic_bf16.hip is the bf16 one; the fp16 modes are refused for these shapes.  The
// inference entry point has no workspace argument in the ABI, so the library keeps scratch blocks per (device, stream) for it
// (host_state.hip generic_arena: allocated on first use, grown when needed -- not inside a graph capture).
#include <algorithm>
#include <vector>

#include "mlp_device.h"
#include "mlp_generic.h"
#include "mlp_generic_kernels.h"
#include "mlp_generic_walk.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- GEMM
struct GemmArgs {
    const float* A; long long a_rs, a_cs;
    const float* B; long long b_rs, b_cs;
    float* C; long long c_rs, c_cs;
    const float* bias;                         // per column n, or NULL
    const float* mask; long long mask_rs;      // C(m,n) *= (mask[m * mask_rs + n] > 0), or NULL (ReLU gate of the backward)
    int M, N, K;
    int relu, accumulate;
    long long k_chunk;                         // split-K: blockIdx.z owns k in [z * k_chunk, min(K, (z+1) * k_chunk)) and writes
    long long split_stride;                    // C + z * split_stride (a partial-sum buffer); 0 = no split
};

constexpr int kBK = 32, kPad = 1;

// Accumulators -> C (+ bias, + C, ReLU, gate).  D layout: lane (i = column, h), register r -> row (r & 3) + 8 (r >> 2) + 4 h of the 32 x 32
// tile.  A tile that lies wholly inside the matrix takes the branch-free path: the sixteen values of a register tile are read (C to add
// to, the gate) in one batch, then computed, then stored -- with a bounds test per element every read was its own exec-masked block
// and waited for its own round trip (64 of them per thread in the input-gradient products of the backward).
template <int TM, int TN>
__device__ __forceinline__ void write_tile(const f32x16 (&acc)[TM][TN], const GemmArgs& g, float* C, int m0, int n0, int wm, int wn, int i,
                                           int h) {
    const bool whole = m0 + 64 * TM <= g.M && n0 + 64 * TN <= g.N;
    if (whole) {
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const long long n = n0 + wn + 32 * tn + i;
            const float bias = g.bias ? g.bias[n] : 0.0f;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) {
                const long long m_first = m0 + wm + 32 * tm + 4 * h;
                float* const dst = C + m_first * g.c_rs + n * g.c_cs;
                const float* const gate = g.mask ? g.mask + m_first * g.mask_rs + n : nullptr;
                float old[16], open[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long dm = (r & 3) + 8 * (r >> 2);
                    old[r] = g.accumulate ? dst[dm * g.c_rs] : 0.0f;
                    open[r] = gate ? gate[dm * g.mask_rs] : 1.0f;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long dm = (r & 3) + 8 * (r >> 2);
                    float v = acc[tm][tn][r] + bias;
                    if (g.accumulate) v += old[r];
                    if (g.relu) v = fmaxf(v, 0.0f);
                    if (g.mask) v = open[r] > 0.0f ? v : 0.0f;
                    dst[dm * g.c_rs] = v;
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
                float* dst = C + m * g.c_rs + n * g.c_cs;
                if (g.accumulate) v += *dst;
                if (g.relu) v = fmaxf(v, 0.0f);
                if (g.mask) v = g.mask[m * g.mask_rs + n] > 0.0f ? v : 0.0f;
                *dst = v;
            }
    }
}

// BM x BN output tile per 256-thread workgroup = a 2 x 2 grid of waves, each (BM / 2) x (BN / 2) = TM x TN MFMA tiles of 32 x 32.
// <64, 64>: one tile per wave (the round-4 kernel: 0.40 of the fp32 matrix peak at width 512 -- per staged byte and per barrier
// it does a quarter of the matrix work of) <128, 128> (round 5): four tiles per wave, every operand value read from LDS feeds
// two MFMAs, 64 KiB of LDS for the two stages; used wherever the product is at least 128 x 128.
template <int BM, int BN>
__global__ void __launch_bounds__(256, 2) gemm_kernel(GemmArgs g) {
    constexpr int TM = BM / 64, TN = BN / 64;
    constexpr int LA = BM * kBK / 256, LB = BN * kBK / 256;      // elements of a stage per thread
    __shared__ float As[2][kBK][BM + kPad];
    __shared__ float Bs[2][kBK][BN + kPad];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // tile of this workgroup.  Workgroups go to the eight XCDs in turn (linear id mod 8) and every XCD has its own L2: with the
    // plain (x = n tile, y = m tile) order the n tiles of one row block -- which all read the same rows of A -- land on different
    // XCDs and A comes from HBM once per n tile (4 x at width 512).  When the m tiles divide by eight, XCD x takes the row blocks
    // congruent to x and walks their n tiles one after the other: A's rows are fetched once and hit in that XCD's L2 afterwards.
    int tile_m = blockIdx.y, tile_n = blockIdx.x;
    if ((gridDim.y & 7u) == 0) {
        const unsigned linear = blockIdx.y * gridDim.x + blockIdx.x, xcd = linear & 7u, idx = linear >> 3;
        tile_m = (int)((idx / gridDim.x) * 8u + xcd);
        tile_n = (int)(idx % gridDim.x);
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const long long k_lo = g.split_stride ? (long long)blockIdx.z * g.k_chunk : 0;
    const long long k_hi = g.split_stride ? (k_lo + g.k_chunk < g.K ? k_lo + g.k_chunk : g.K) : g.K;
    float* C = g.C + (g.split_stride ? (long long)blockIdx.z * g.split_stride : 0);

    // thread -> elements of a stage: LA of A (BM x kBK) and LB of B (kBK x BN), walking the contiguous dimension first.
    // Element e of a thread sits a FIXED step from element e - 1, in memory and in LDS: one 32-bit byte offset per operand and
    // thread (computed once), a wave-uniform base per stage and element (scalar arithmetic), immediate LDS offsets.  (Round 4
    // computed m * a_rs + k * a_cs in 64 bits per element and stage: 1 021 vector instructions beside 16 MFMAs, 2 785 beside 64
    // in the first 128 x 128 build -- the kernel was bound by its address arithmetic, not by the matrix pipe.)
    const bool a_m_major = g.a_rs == 1;        // A contiguous along m (the transposed operand of the weight gradient)
    const bool b_n_major = g.b_cs == 1;
    const int a_m = a_m_major ? (tid & (BM - 1)) : (tid / kBK), a_k = a_m_major ? (tid / BM) : (tid & (kBK - 1));
    const int a_dm = a_m_major ? 0 : 256 / kBK, a_dk = a_m_major ? 256 / BM : 0;            // element e + 1 relative to e
    const int b_n = b_n_major ? (tid & (BN - 1)) : (tid / kBK), b_k = b_n_major ? (tid / BN) : (tid & (kBK - 1));
    const int b_dn = b_n_major ? 0 : 256 / kBK, b_dk = b_n_major ? 256 / BN : 0;
    const unsigned a_byte = (unsigned)((long long)a_m * g.a_rs + (long long)a_k * g.a_cs) * 4u;   // (a_m < BM, a_k < 32: fits)
    const unsigned b_byte = (unsigned)((long long)b_k * g.b_rs + (long long)b_n * g.b_cs) * 4u;
    // (a thread's elements span < 16 steps of at most 8 rows or 4 k-columns: byte offsets inside the tile stay far below 2^31
    // for any row length the activation matrix can have)
    const unsigned a_step32 = (unsigned)(((long long)a_dm * g.a_rs + (long long)a_dk * g.a_cs) * 4);
    const unsigned b_step32 = (unsigned)(((long long)b_dk * g.b_rs + (long long)b_dn * g.b_cs) * 4);
    const int m_left = g.M - m0, n_left = g.N - n0;           // rows / columns of the tile inside the matrix
    const char* const a_tile = reinterpret_cast<const char*>(g.A + (long long)m0 * g.a_rs);
    const char* const b_tile = reinterpret_cast<const char*>(g.B + (long long)n0 * g.b_cs);
    float ra[LA], rb[LB];
    unsigned a_inside = 0, b_inside = 0;      // bit e: element e of the stage in flight lies inside the matrix
    auto load_stage = [&](long long k0) {
        const char* a_stage = a_tile + k0 * g.a_cs * 4;
        const char* b_stage = b_tile + k0 * g.b_rs * 4;
        const int k_left = (int)(k_hi - k0 < kBK ? k_hi - k0 : kBK);       // 32 except in the last stage of a ragged K
        // branch-free: an element outside the matrix reads the stage's first element (always inside) and is replaced by zero
        // WHEN IT IS STORED, after this stage's MFMAs (a predicated load per element compiles to one exec-masked basic block per
        // load, and a select right here makes the MFMAs wait for the loads they are meant to hide)
        a_inside = b_inside = 0;
#pragma unroll
        for (int e = 0; e < LA; ++e) {
            const bool inside = a_m + e * a_dm < m_left && a_k + e * a_dk < k_left;
            a_inside |= inside ? 1u << e : 0u;
            ra[e] = *reinterpret_cast<const float*>(a_stage + (inside ? a_byte + (unsigned)e * a_step32 : 0u));
        }
#pragma unroll
        for (int e = 0; e < LB; ++e) {
            const bool inside = b_n + e * b_dn < n_left && b_k + e * b_dk < k_left;
            b_inside |= inside ? 1u << e : 0u;
            rb[e] = *reinterpret_cast<const float*>(b_stage + (inside ? b_byte + (unsigned)e * b_step32 : 0u));
        }
    };
    float* const as0 = &As[0][a_k][a_m];
    float* const bs0 = &Bs[0][b_k][b_n];
    const int as_step = a_dk * (BM + kPad) + a_dm, bs_step = b_dk * (BN + kPad) + b_dn;
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int e = 0; e < LA; ++e) as0[buf * (kBK * (BM + kPad)) + e * as_step] = (a_inside >> e) & 1u ? ra[e] : 0.0f;
#pragma unroll
        for (int e = 0; e < LB; ++e) bs0[buf * (kBK * (BN + kPad)) + e * bs_step] = (b_inside >> e) & 1u ? rb[e] : 0.0f;
    };

    // wave (wm, wn) owns a (32 TM) x (32 TN) sub-tile; MFMA operands: A(m = lane & 31, k = lane >> 5), B(k = lane >> 5, n = lane & 31)
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
        store_stage(0);
        __syncthreads();
        int buf = 0;
        for (long long k0 = k_lo; k0 < k_hi; k0 += kBK) {
            const bool more = k0 + kBK < k_hi;
            if (more) load_stage(k0 + kBK);                     // in flight during this stage's MFMAs
            const float* a_rd = &As[buf][h][wm + i];
            const float* b_rd = &Bs[buf][h][wn + i];
            // the operands of k-pair p + 1 are requested BEFORE the MFMAs of pair p are issued (two register sets; the scheduling
            // barrier keeps the compiler from sinking the reads back to their use): left alone it emitted read, wait, four MFMAs,
            // read, wait ... with one register set, and the matrix pipe sat idle for an LDS round trip per pair -- 0.54 busy (PMC,
            // profiles/r05_pmc_layered_gemm.json), 0.50 of the peak
            float av[2][TM], bv[2][TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) av[0][tm] = a_rd[32 * tm];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) bv[0][tn] = b_rd[32 * tn];
#pragma unroll
            for (int p = 0; p < kBK / 2; ++p) {
                if (p + 1 < kBK / 2) {
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) av[(p + 1) & 1][tm] = a_rd[2 * (p + 1) * (BM + kPad) + 32 * tm];
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) bv[(p + 1) & 1][tn] = b_rd[2 * (p + 1) * (BN + kPad) + 32 * tn];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p & 1][tm], bv[p & 1][tn], acc[tm][tn], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (more) {
                store_stage(buf ^ 1);
                __syncthreads();
                buf ^= 1;
            }
        }
    }
    write_tile<TM, TN>(acc, g, C, m0, n0, wm, wn, i, h);
}


// How an operand tile (TILE rows of m resp. n  x  kBK of k) gets from memory into LDS.  `st` = stride (floats) between neighbouring
// m resp. n, `sk` = between neighbouring k.
//   (element by element, any strides: gemm_kernel above -- one dword load and one ds_write_b32 per element; kept as written in
//    rounds 4-5: the same staging expressed through this struct compiled to the same instructions and ran 3-4 % slower)
//   MODE 1: sk == 1 -- 16-byte groups along k: four k of one row per load, four ds_write_b32 (row stride TILE + 1: conflict-free);
//   MODE 2: st == 1 -- 16-byte groups along m / n: four neighbours of one k per load, ONE ds_write_b128 (row stride TILE + 4).
// Round 5: with MODE 0 everywhere the staging cost 50 % on top of the MFMA loop (profiles/r05_layered_ablation.txt); every product
// of the layered path has a contiguous direction in each operand, so launch_gemm picks MODE 1 / 2 whenever strides, sizes and
// addresses are multiples of four floats, and gemm_kernel otherwise (ragged K such as the 63-wide encoding, odd row counts).
template <int TILE, int MODE>
struct Stager {
    static_assert(MODE == 1 || MODE == 2, "16-byte staging only");
    static constexpr int kRow = TILE + (MODE == 2 ? 4 : 1);            // floats per k-row of the tile in LDS
    static constexpr int kElems = TILE * kBK / 256;                      // floats per thread and stage
    static constexpr int kGroups = kElems / 4;                           // 16-byte groups per thread and stage
    static constexpr int kStepK2 = 256 / (TILE / 4);                     // MODE 2: k rows covered per pass of the 256 threads
    const char* tile;            // first element of the tile at k = 0
    long long sk_bytes;
    int left;                    // rows (m resp. n) of the tile inside the matrix
    int t0, k0;                  // this thread's first group: tile index, k index of its first element
    int dt, dk;                  // step to the thread's next group
    unsigned byte0, step;        // byte offset of the first element / group inside a stage, and to the next one
    unsigned inside;             // bit e: element / group e of the stage in flight lies inside the matrix
    float r[kElems];
    int lds0, lds_step;          // float offset of the first element inside a stage buffer, and to the next one

    __device__ __forceinline__ void init(const float* first, long long st, long long sk, int left_, int tid) {
        tile = reinterpret_cast<const char*>(first);
        sk_bytes = sk * 4;
        left = left_;
        inside = 0;
        if constexpr (MODE == 1) {
            t0 = tid >> 3; k0 = (tid & 7) * 4; dt = 32; dk = 0;
            byte0 = (unsigned)((long long)t0 * st + k0) * 4u;
            step = (unsigned)(32 * st * 4);
            lds0 = k0 * kRow + t0;
            lds_step = 32;
        } else {
            t0 = (tid & (TILE / 4 - 1)) * 4; k0 = tid / (TILE / 4); dt = 0; dk = kStepK2;
            byte0 = (unsigned)((long long)k0 * sk + t0) * 4u;
            step = (unsigned)(kStepK2 * sk * 4);
            lds0 = k0 * kRow + t0;
            lds_step = kStepK2 * kRow;
        }
    }
    // branch-free: an element outside the matrix reads the stage's first element (always inside) and is replaced by zero WHEN IT
    // IS STORED, after this stage's MFMAs (a predicated load per element compiles to one exec-masked basic block per load, and a
    // select right here makes the MFMAs wait for the loads they are meant to hide)
    __device__ __forceinline__ void load(long long k_first, int k_left) {
        const char* stage = tile + k_first * sk_bytes;
        inside = 0;
#pragma unroll
        for (int e = 0; e < kGroups; ++e) {
            const bool in = t0 + e * dt < left && k0 + e * dk < k_left;      // (sizes are multiples of four: all four or none)
            inside |= in ? 1u << e : 0u;
            const f32x4 v = *reinterpret_cast<const f32x4*>(stage + (in ? byte0 + (unsigned)e * step : 0u));
#pragma unroll
            for (int q = 0; q < 4; ++q) r[4 * e + q] = v[q];
        }
    }
    __device__ __forceinline__ void store(float* buffer) {
        if constexpr (MODE == 1) {
#pragma unroll
            for (int e = 0; e < kGroups; ++e)
#pragma unroll
                for (int q = 0; q < 4; ++q) buffer[lds0 + e * lds_step + q * kRow] = (inside >> e) & 1u ? r[4 * e + q] : 0.0f;
        } else {
#pragma unroll
            for (int e = 0; e < kGroups; ++e) {
                const bool in = (inside >> e) & 1u;
                const f32x4 v = {in ? r[4 * e] : 0.0f, in ? r[4 * e + 1] : 0.0f, in ? r[4 * e + 2] : 0.0f, in ? r[4 * e + 3] : 0.0f};
                *reinterpret_cast<f32x4*>(buffer + lds0 + e * lds_step) = v;
            }
        }
    }
};

// BM x BN output tile per 256-thread workgroup = a 2 x 2 grid of waves, each (BM / 2) x (BN / 2) = TM x TN MFMA tiles of 32 x 32.
// <64, 64>: one tile per wave (the round-4 kernel: 0.40 of the fp32 matrix peak at width 512 -- per staged byte and per barrier
// it does a quarter of the matrix work of) <128, 128> (round 5): four tiles per wave, every operand value read from LDS feeds
// two MFMAs, 64 KiB of LDS for the two stages; used wherever the product is at least 128 x 128.  AV / BV: Stager modes.
template <int BM, int BN, int AV, int BV>
__global__ void __launch_bounds__(256, 2) gemm_vec_kernel(GemmArgs g) {
    static_assert(AV > 0 && BV > 0, "element-by-element staging is gemm_kernel's");
    constexpr int TM = BM / 64, TN = BN / 64;
    using StageA = Stager<BM, AV>;
    using StageB = Stager<BN, BV>;
    constexpr int SA = StageA::kRow, SB = StageB::kRow;
    __shared__ __attribute__((aligned(16))) float As[2][kBK * SA];
    __shared__ __attribute__((aligned(16))) float Bs[2][kBK * SB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // PERSISTENT workgroups: the grid is two per CU (launch_gemm) and a workgroup walks tiles `blockIdx.x, + gridDim.x, ...` of the
    // tile sequence below -- the first stage of its NEXT tile is requested before the accumulators of this one are written out, so
    // that neither the first loads' round trip nor the epilogue's stores stand alone between two tiles' MFMAs (the two workgroups of
    // a CU run in step: what one tile spent outside its MFMA loop nobody covered -- 85 us per pair of tiles against 55 of matrix
    // work, profiles/r05_layered_ablation.txt).
    // Tile sequence.  Workgroups go to the eight XCDs in turn (linear id mod 8; the grid is a multiple of eight, so a workgroup stays
    // on its XCD's residue) and every XCD has its own L2: with the plain (n tile fastest) order the n tiles of one row block -- which
    // all read the same rows of A -- land on different XCDs and A comes from HBM once per n tile (4 x at width 512).  When the m tiles
    // divide by eight, XCD x takes the row blocks congruent to x and walks their n tiles one after the other: A's rows are fetched
    // once and hit in that XCD's L2 afterwards.
    const unsigned tiles_n = (unsigned)((g.N + BN - 1) / BN), tiles_m = (unsigned)((g.M + BM - 1) / BM), tiles = tiles_n * tiles_m;
    auto tile_of = [&](unsigned linear_id, int* m_first, int* n_first) {
        unsigned tile_m = linear_id / tiles_n, tile_n = linear_id % tiles_n;
        if ((tiles_m & 7u) == 0) {
            const unsigned xcd = linear_id & 7u, idx = linear_id >> 3;
            tile_m = (idx / tiles_n) * 8u + xcd;
            tile_n = idx % tiles_n;
        }
        *m_first = (int)tile_m * BM;
        *n_first = (int)tile_n * BN;
    };
    unsigned linear = blockIdx.x;
    if (linear >= tiles) return;
    int m0, n0;
    tile_of(linear, &m0, &n0);
    const long long k_lo = g.split_stride ? (long long)blockIdx.z * g.k_chunk : 0;
    const long long k_hi = g.split_stride ? (k_lo + g.k_chunk < g.K ? k_lo + g.k_chunk : g.K) : g.K;
    float* C = g.C + (g.split_stride ? (long long)blockIdx.z * g.split_stride : 0);

    // thread -> elements of a stage, walking the contiguous dimension first: a thread's elements sit a FIXED step apart in memory and
    // in LDS -- one 32-bit byte offset per operand and thread (computed once), a wave-uniform base per stage (scalar arithmetic),
    // immediate LDS offsets.  (Round 4 computed m * a_rs + k * a_cs in 64 bits per element and stage: 1 021 vector instructions
    // beside 16 MFMAs -- the kernel was bound by its address arithmetic, not by the matrix pipe.)
    StageA sa;
    StageB sb;
    sa.init(g.A + (long long)m0 * g.a_rs, g.a_rs, g.a_cs, g.M - m0, tid);
    sb.init(g.B + (long long)n0 * g.b_cs, g.b_cs, g.b_rs, g.N - n0, tid);
    auto load_stage = [&](long long k0) {
        const int k_left = (int)(k_hi - k0 < kBK ? k_hi - k0 : kBK);       // 32 except in the last stage of a ragged K
        sa.load(k0, k_left);
        sb.load(k0, k_left);
    };
    auto store_stage = [&](int buf) {
        sa.store(As[buf]);
        sb.store(Bs[buf]);
    };

    // wave (wm, wn) owns a (32 TM) x (32 TN) sub-tile; MFMA operands: A(m = lane & 31, k = lane >> 5), B(k = lane >> 5, n = lane & 31)
    const int wm = (wave >> 1) * (32 * TM), wn = (wave & 1) * (32 * TN), i = lane & 31, h = lane >> 5;
    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.0f;
    const bool any_k = k_lo < k_hi;
    if (any_k) load_stage(k_lo);
    while (true) {
        if (any_k) {
            store_stage(0);
            __syncthreads();
            int buf = 0;
            for (long long k0 = k_lo; k0 < k_hi; k0 += kBK) {
                const bool more = k0 + kBK < k_hi;
                if (more) load_stage(k0 + kBK);                     // in flight during this stage's MFMAs
                const float* a_rd = &As[buf][h * SA + wm + i];
                const float* b_rd = &Bs[buf][h * SB + wn + i];
                // the operands of k-pair p + 1 are requested BEFORE the MFMAs of pair p are issued (two register sets; the scheduling
                // barrier keeps the compiler from sinking the reads back to their use): left alone it emitted read, wait, four MFMAs,
                // read, wait ... with one register set, and the matrix pipe sat idle for an LDS round trip per pair -- 0.54 busy (PMC,
                // profiles/r05_pmc_layered_gemm.json), 0.50 of the peak
                float av[2][TM], bv[2][TN];
    #pragma unroll
                for (int tm = 0; tm < TM; ++tm) av[0][tm] = a_rd[32 * tm];
    #pragma unroll
                for (int tn = 0; tn < TN; ++tn) bv[0][tn] = b_rd[32 * tn];
    #pragma unroll
                for (int p = 0; p < kBK / 2; ++p) {
                    if (p + 1 < kBK / 2) {
    #pragma unroll
                        for (int tm = 0; tm < TM; ++tm) av[(p + 1) & 1][tm] = a_rd[2 * (p + 1) * SA + 32 * tm];
    #pragma unroll
                        for (int tn = 0; tn < TN; ++tn) bv[(p + 1) & 1][tn] = b_rd[2 * (p + 1) * SB + 32 * tn];
                    }
                    __builtin_amdgcn_sched_barrier(0);
    #pragma unroll
                    for (int tm = 0; tm < TM; ++tm)
    #pragma unroll
                        for (int tn = 0; tn < TN; ++tn)
                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p & 1][tm], bv[p & 1][tn], acc[tm][tn], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (more) {
                    store_stage(buf ^ 1);
                    __syncthreads();
                    buf ^= 1;
                }
            }
            __syncthreads();          // (every wave is done reading the buffers before the next tile's first stage overwrites buffer 0)
        }
        // the next tile's first stage, in flight while this tile's accumulators go out
        const unsigned next = linear + gridDim.x;
        int m_next = 0, n_next = 0;
        if (next < tiles) {
            tile_of(next, &m_next, &n_next);
            sa.init(g.A + (long long)m_next * g.a_rs, g.a_rs, g.a_cs, g.M - m_next, tid);
            sb.init(g.B + (long long)n_next * g.b_cs, g.b_cs, g.b_rs, g.N - n_next, tid);
            if (any_k) load_stage(k_lo);
        }
        write_tile<TM, TN>(acc, g, C, m0, n0, wm, wn, i, h);
        if (next >= tiles) break;
        linear = next; m0 = m_next; n0 = n_next;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.0f;
    }
}

// The same sums for rows of whole 16-byte groups (ld and cols multiples of 4, dz 16-byte aligned: every Linear layer but the
// heads).  Round 5: the scalar kernel above kept ONE 256-byte load per wave in flight -- 614 us per call at 262 144 x 512, 0.9 TB/s,
// 17 % of the layered backward (rocprofv3, profiles/r05_layered_kernel_stats.csv).  Here a lane owns four columns, a wave 256, the
// eight waves of a workgroup take the rows of their chunk in turn, eight rows (8 KiB per wave) in flight; a lane adds its rows in
// order, the waves' sums are added in wave order: fixed, whatever the timing.
__global__ void __launch_bounds__(512) colsum4_kernel(const float* __restrict__ dz, long long ld, long long rows, int cols,
                                                      long long rows_per_split, float* __restrict__ partial) {
    constexpr int kParts = 8, kAhead = 8;
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * 4;
    const long long lo = (long long)blockIdx.y * rows_per_split, hi = lo + rows_per_split < rows ? lo + rows_per_split : rows;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    if (col < cols) {
        const float* base = dz + col;
        long long r = lo + part;
        for (; r + (long long)(kAhead - 1) * kParts < hi; r += (long long)kAhead * kParts) {
            f32x4 v[kAhead];
#pragma unroll
            for (int e = 0; e < kAhead; ++e) v[e] = *reinterpret_cast<const f32x4*>(base + (r + (long long)e * kParts) * ld);
#pragma unroll
            for (int e = 0; e < kAhead; ++e) s += v[e];
        }
        for (; r < hi; r += kParts) s += *reinterpret_cast<const f32x4*>(base + r * ld);
    }
    __shared__ f32x4 sh[kParts][64];
    sh[part][lane] = s;
    __syncthreads();
    if (part == 0 && col < cols) {
        f32x4 t = sh[0][lane];
#pragma unroll
        for (int q = 1; q < kParts; ++q) t += sh[q][lane];
        *reinterpret_cast<f32x4*>(partial + (long long)blockIdx.y * cols + col) = t;
    }
}

__global__ void __launch_bounds__(256) copy_kernel(float* __restrict__ dst, const float* __restrict__ src, long long count) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------------------ host side
int launch_gemm(const GemmArgs& g, int splits, hipStream_t s) {
    if (g.M <= 0 || g.N <= 0) return SNERF_OK;
    int tile = 0;
    const dim3 grid = gemm_grid(g.M, g.N, splits, &tile);
    if (tile == 128) {
        // 16-byte staging (Stager MODE 1 / 2) where everything it touches is a multiple of four floats; the three combinations are
        // the path's three products: forward (A, B along k), input gradient (A along k, B along n), weight gradient (A along m,
        // B along n)
        const bool k_fours = g.K % 4 == 0 && (splits <= 0 || g.k_chunk % 4 == 0);
        const bool a_along_k = g.a_cs == 1 && g.a_rs % 4 == 0 && aligned16(g.A) && k_fours;
        const bool a_along_m = g.a_rs == 1 && g.a_cs % 4 == 0 && aligned16(g.A) && g.M % 4 == 0;
        const bool b_along_k = g.b_rs == 1 && g.b_cs % 4 == 0 && aligned16(g.B) && k_fours;
        const bool b_along_n = g.b_cs == 1 && g.b_rs % 4 == 0 && aligned16(g.B) && g.N % 4 == 0;
        // (persistent workgroups: two per CU of the current device, a multiple of eight so that a workgroup's tiles stay on its XCD)
        const unsigned tiles = grid.x * grid.y;
        const dim3 walkers(std::min(tiles, snerf::persistent_workgroups()), 1, grid.z);
        if (a_along_k && b_along_k) hipLaunchKernelGGL((gemm_vec_kernel<128, 128, 1, 1>), walkers, dim3(256), 0, s, g);
        else if (a_along_k && b_along_n) hipLaunchKernelGGL((gemm_vec_kernel<128, 128, 1, 2>), walkers, dim3(256), 0, s, g);
        else if (a_along_m && b_along_n) hipLaunchKernelGGL((gemm_vec_kernel<128, 128, 2, 2>), walkers, dim3(256), 0, s, g);
        else hipLaunchKernelGGL((gemm_kernel<128, 128>), grid, dim3(256), 0, s, g);
    } else {
        hipLaunchKernelGGL((gemm_kernel<64, 64>), grid, dim3(256), 0, s, g);
    }
    return snerf::check_launch("mlp_generic(gemm)");
}

// The fp32 operand format of the layer walk (mlp_generic_walk.h): activation row and dZ buffers of floats, every block a layer reads
// at a multiple of four floats (so that the GEMM can stage it 16 bytes at a time, Stager MODE 1 / 2), the heads in the row.
struct F32Operands {
    using Act = float;
    static constexpr const char* kName = "mlp_generic";
    static constexpr int kAlign = 4;
    static constexpr bool kHeadsInRow = true;
    static long long ld(long long width) { return width; }
    static long long floats(long long elems) { return elems; }

    // Y[rows, out] = act(X[rows, in] . W[out, in]^T + b): X, Y are column blocks of the activation matrix
    static int linear(const float* x, long long x_rs, float* y, long long y_rs, long long rows, int in, int out, const float* w,
                      const float* b, bool relu, hipStream_t s) {
        GemmArgs g = {};
        g.A = x; g.a_rs = x_rs; g.a_cs = 1;
        g.B = w; g.b_rs = 1; g.b_cs = in;
        g.C = y; g.c_rs = y_rs; g.c_cs = 1;
        g.bias = b; g.M = (int)rows; g.N = out; g.K = in; g.relu = relu ? 1 : 0;
        return launch_gemm(g, 0, s);
    }
    static int input_grad(const float* dz, long long dz_ld, int out, const float* w, int w_ld, int cols, float* dx, long long dx_ld,
                          bool add, const float* gate, long long gate_rs, long long rows, hipStream_t s) {
        GemmArgs g = {};
        g.A = dz; g.a_rs = dz_ld; g.a_cs = 1;
        g.B = w; g.b_rs = w_ld; g.b_cs = 1;
        g.C = dx; g.c_rs = dx_ld; g.c_cs = 1;
        g.M = (int)rows; g.N = cols; g.K = out; g.accumulate = add ? 1 : 0;
        g.mask = gate; g.mask_rs = gate_rs;
        return launch_gemm(g, 0, s);
    }
    static int wgrad_gemm(const float* dz, long long dz_ld, int out, const float* x, long long x_rs, int in, long long total, int splits,
                          long long k_chunk, float* partial, hipStream_t s) {
        GemmArgs g = {};
        g.A = dz; g.a_rs = 1; g.a_cs = dz_ld;           // A(m = out feature, k = sample) = dZ[k][m]
        g.B = x; g.b_rs = x_rs; g.b_cs = 1;             // B(k = sample, n = in feature)
        g.C = partial; g.c_rs = in; g.c_cs = 1;
        g.M = out; g.N = in; g.K = (int)total; g.k_chunk = k_chunk; g.split_stride = (long long)out * in;
        return launch_gemm(g, splits, s);
    }
    static int colsum(const float* dz, long long dz_ld, int out, long long total, int bsplits, long long b_chunk, float* bpart, hipStream_t s) {
        if (out % 4 == 0 && dz_ld % 4 == 0 && aligned16(dz) && aligned16(bpart))
            hipLaunchKernelGGL(colsum4_kernel, dim3((out + 255) / 256, bsplits), dim3(512), 0, s, dz, dz_ld, total, out, b_chunk, bpart);
        else
            hipLaunchKernelGGL(colsum_kernel, dim3((out + 63) / 64, bsplits), dim3(256), 0, s, dz, dz_ld, total, out, b_chunk, bpart);
        return SNERF_OK;
    }
};

// fp32 or bf16 operands ('bf16s8' is 'bf16' here: the fp8 saved trunk exists for the fused 256-wide kernels only): *bf16 says which.
// The fp16 modes are refused for these shapes, not run in another precision.
int layered_operands(const GenericPlan& p, int precision, const char* entry, bool* bf16) {
    *bf16 = precision == SNERF_PRECISION_BF16 || precision == SNERF_PRECISION_BF16S8;
    if (precision == SNERF_PRECISION_FP32 || *bf16) return SNERF_OK;
    return snerf::fail(SNERF_E_UNSUPPORTED, "%s: this MLP shape (width %d, views %d x %d) runs on the layered path, in fp32 or bf16 "
                                            "operands; hip_precision must be 'fp32' or 'bf16'/'bf16s8'", entry, p.width, p.views_depth,
                       p.views_width);
}

}  // namespace

namespace snerf {

int generic_plan(const snerf_mlp_desc* d, GenericPlan* out) {
    if (!d) return fail(SNERF_E_INVALID, "mlp: NULL descriptor");
    GenericPlan p;
    p.depth = d->points_net_depth; p.width = d->points_net_width;
    p.view_dep = d->view_dependent_rgb != 0;
    p.views_depth = p.view_dep ? d->views_net_depth : 0;
    p.views_width = p.view_dep ? d->views_net_width : 0;
    p.points_degree = d->points_pe_degree; p.views_degree = p.view_dep ? d->views_pe_degree : 0;
    if (p.width < 1 || p.width > 4096) return fail(SNERF_E_UNSUPPORTED, "mlp: points_net_width %d outside 1..4096", p.width);
    if (p.depth < 1 || p.depth == 5 || p.depth > 64)
        return fail(SNERF_E_UNSUPPORTED, "mlp: points_net_depth %d unsupported (the reference itself cannot build depth 5: the skip "
                                         "concat would feed pts_output_linear)", p.depth);
    if (p.points_degree < 1 || p.points_degree > 16) return fail(SNERF_E_UNSUPPORTED, "mlp: points positional-encoding degree %d outside 1..16", p.points_degree);
    if (d->predict_visibility) return fail(SNERF_E_UNSUPPORTED, "mlp: predict_visibility is built for the fused shapes only (widths 128/256, views 64/128)");
    if (p.view_dep) {
        if (!d->use_view_dirs) return fail(SNERF_E_UNSUPPORTED, "mlp: view_dependent_rgb without use_view_dirs");
        if (p.views_depth < 1 || p.views_depth > 16) return fail(SNERF_E_UNSUPPORTED, "mlp: views_net_depth %d outside 1..16", p.views_depth);
        if (p.views_width < 1 || p.views_width > 4096) return fail(SNERF_E_UNSUPPORTED, "mlp: views_net_width %d outside 1..4096", p.views_width);
        if (p.views_degree < 1 || p.views_degree > 16) return fail(SNERF_E_UNSUPPORTED, "mlp: views positional-encoding degree %d outside 1..16", p.views_degree);
    }
    p.pe_full = 3 + 6 * p.points_degree;
    p.pts_in = p.pe_full;
    if (d->sigma_pe_degree >= 0) {
        if (d->sigma_pe_degree > p.points_degree) return fail(SNERF_E_UNSUPPORTED, "mlp: sigma encoding degree %d exceeds the points degree %d", d->sigma_pe_degree, p.points_degree);
        if (!p.view_dep) return fail(SNERF_E_UNSUPPORTED, "mlp: points_sigma_positional_encoding_degree needs view-dependent colour");
        p.pts_in = (2 * d->sigma_pe_degree + 1) * 3;
    }
    p.extra = p.pe_full - p.pts_in;
    p.views_pe = p.view_dep ? 3 + 6 * p.views_degree : 0;
    p.views_in = p.width + p.extra + p.views_pe;
    p.pts_out_rows = p.view_dep ? 1 : 4;
    p.num_params = 2 * p.depth + 2 + (p.view_dep ? 2 + 2 * p.views_depth + 2 : 0);
    // parameter offsets in the "packed" buffer (a plain concatenation in ABI order)
    long long off = 0;
    auto param = [&](long long count) { p.w_off.push_back(off); p.w_count.push_back(count); off += (count + 3) / 4 * 4; };
    for (int l = 0; l < p.depth; ++l) { param((long long)p.width * p.layer_in_dim(l)); param(p.width); }
    param((long long)p.pts_out_rows * p.width); param(p.pts_out_rows);
    if (p.view_dep) {
        param((long long)p.width * p.width); param(p.width);
        for (int j = 0; j < p.views_depth; ++j) { param((long long)p.views_width * (j == 0 ? p.views_in : p.views_width)); param(p.views_width); }
        param(3LL * p.views_width); param(3);
    }
    p.packed_floats = off;
    p.row = generic_row(p, F32Operands::kAlign, F32Operands::kHeadsInRow).row;
    *out = p;
    return SNERF_OK;
}

GenericRow generic_row(const GenericPlan& p, int align, bool heads_in_row) {
    GenericRow r;
    int c = 0;
    auto next = [&]() { c = (c + align - 1) / align * align; };
    r.c_pe = c; c += p.pe_full;
    next(); r.c_pev = c; c += p.views_pe;
    r.c_h.assign(p.depth, 0);
    for (int l = 0; l < p.depth; ++l) {
        next();
        if (l == 4 && p.depth > 5) { r.c_x5 = c; c += p.pts_in; }      // [encoding | H_4]: the skip layer's input (:662-663)
        r.c_h[l] = c; c += p.width;
    }
    next(); r.c_v0 = c; if (p.view_dep) c += p.views_in;
    r.c_hv.assign(p.views_depth, 0);
    for (int j = 0; j < p.views_depth; ++j) { next(); r.c_hv[j] = c; c += p.views_width; }
    next();
    if (heads_in_row) { r.c_out = c; r.c_vout = c + 4; c += 8; r.head_rs = c; }
    r.row = c;
    return r;
}

int generic_pack(const GenericPlan& p, const float* const* params, float* packed, hipStream_t s) {
    for (int i = 0; i < p.num_params; ++i) {
        hipLaunchKernelGGL(copy_kernel, dim3(stride_grid(p.w_count[i], 256)), dim3(256), 0, s, packed + p.w_off[i], params[i], p.w_count[i]);
        const int rc = check_launch("mlp_pack(layered)");
        if (rc != SNERF_OK) return rc;
    }
    return SNERF_OK;
}

size_t generic_saved_floats(const GenericPlan& p, long long total) { return (size_t)total * (size_t)p.row; }

int generic_forward(const GenericPlan& p, const float* packed, const float* origins, const float* dirs, const float* view_dirs,
                    const float* depths, long long num_rays, int num_samples, const float* noise, float* sigma, float* rgb,
                    float* saved_acts, int precision, hipStream_t s) {
    bool bf16 = false;
    const int rc = layered_operands(p, precision, "mlp_forward", &bf16);
    if (rc != SNERF_OK) return rc;
    ProfileScope timed(SNERF_PROFILE_MLP_FORWARD, s, num_rays * num_samples);
    auto call = bf16 ? generic_forward_bf16 : forward_call<F32Operands>;
    return call(p, packed, origins, dirs, view_dirs, depths, num_rays, num_samples, noise, sigma, rgb, saved_acts, s);
}

size_t generic_backward_workspace_floats(const GenericPlan& p, long long total) { return (size_t)(workspace_of<F32Operands>(p, total).end + 64); }

int generic_backward(const GenericPlan& p, const float* packed, const float* acts, const float* sigma, const float* rgb,
                     const float* d_sigma, const float* d_rgb, long long total, float* workspace, float* const* grads, int precision,
                     int accumulate, hipStream_t s) {
    bool bf16 = false;
    const int rc = layered_operands(p, precision, "mlp_backward", &bf16);
    if (rc != SNERF_OK) return rc;
    ProfileScope timed(SNERF_PROFILE_MLP_BACKWARD, s, total);
    auto call = bf16 ? generic_backward_bf16 : backward_walk<F32Operands>;
    return call(p, packed, acts, sigma, rgb, d_sigma, d_rgb, total, workspace, grads, accumulate, s);
}

}  // namespace snerf
