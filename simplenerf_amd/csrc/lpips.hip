// Q3: LPIPS (version 0.1) of a rendered frame on the device -- the reference's src/qa/04_LPIPS and 14_MaskedLPIPS, which call
// lpips.LPIPS(net='alex') on the 8-bit frames -- on the AlexNet backbone and on the VGG-16 backbone (net='vgg') that much of the
// literature reports.  The weights come from the caller (snerf_lpips_pack re-orders them once); five fp64 sums leave the device and
// the host divides by each tap's pixel count and adds (simplenerf_amd/qa.py).  Both networks are tables of conv_index.h walked by
// the same code: AlexNet's five convolutions each feed a tap; of VGG-16's thirteen, five do.
//
//   prepare      both uint8 (h,w,3) images -> one fp32 NHWC tensor (2,h,w,3), gt first: x = u * 2 / 255 - 1 in that fp32 order
//                (the package's im2tensor), then (x - shift) / scale; with a mask, eval = mask ? eval : gt on the bytes first
//   conv         conv + bias + ReLU as an implicit GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32): rows = output pixels of
//                both images, columns = output channels, k = (tap row, tap column, input channel) -- conv_index.h.  The A operand is
//                gathered from the NHWC activations while a stage is loaded (padding and the tails as zeros): no im2col matrix
//   pool         3 x 3 stride 2 maximum (AlexNet) / 2 x 2 stride 2 maximum (VGG-16), NHWC
//   layer sums   per pixel of a tap: v = sum_c lin_c (f_gt / (|f_gt| + 1e-10) - f_eval / (|f_eval| + 1e-10))^2 in fp32, widened to
//                fp64 and reduced wave -> workgroup -> one partial per workgroup; one last launch folds all five layers
//
// Every sum runs in one fixed order that depends on nothing but the extents (no atomics, no split of K across workgroups): two
// calls return the same bits, and so do the two argument orders (the two images go through the same arithmetic, and (a - b)^2 is
// symmetric).  Bound: the convolutions by the fp32 matrix pipe (10.8 GMAC per 756 x 1008 image for AlexNet, 233 GMAC for VGG-16),
// everything else by memory.
#include <cmath>

#include "block_reduce.h"
#include "conv_index.h"
#include "snerf_common.h"
#include "wave.h"

namespace {

using namespace snerf::conv_index;
using namespace snerf::reduce;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBM = 128, kBN = 64;         // output tile of a workgroup: pixels x channels
constexpr int kARow = kBM + 1;             // LDS row strides (floats): conflict-free ds_write_b32 of a k-column / 16-byte aligned rows
constexpr int kBRow = kBN + 4;
constexpr int kRowsPerThread = kBM * kSlab / kBlock;      // 16 elements of an A stage per thread: one k, 16 rows
constexpr int kMaxPartials = 1024;         // workgroups of a layer's reduction
constexpr int kChains = 4;                 // independent accumulator sets: k-pair p of every slab goes to set p % 4
static_assert(kSlab == 32 && kBlock == 256, "the staging maps one k-column of a slab to every thread");

// ------------------------------------------------------------------------------------------------ packed weights
// A backbone: its convolutions in order, which tap (if any) the ReLU of each feeds, and the max-pool in front of the convolutions
// whose geometry says `pool_before`.  Both networks have five taps.
constexpr int kTaps = 5, kMaxConvs = kVggConvs;
static_assert(kLayers == kTaps && kVggTaps == kTaps && kLayers <= kMaxConvs, "the fold and the sums take five taps");
struct Network {
    const char* name;
    int convs;
    const ConvGeom* geom;
    const int* tap_of;
    int pool_window, min_extent;
};
constexpr int kAlexTapOf[kLayers] = {0, 1, 2, 3, 4};
constexpr Network kNetworks[2] = {{"AlexNet", kLayers, kGeom, kAlexTapOf, kPoolWindow, kMinExtent},
                                  {"VGG-16", kVggConvs, kVggGeom, kVggTapOf, kVggPoolWindow, kVggMinExtent}};
static_assert(SNERF_LPIPS_ALEX == 0 && SNERF_LPIPS_VGG16 == 1, "kNetworks is indexed by the ABI's selector");
static_assert(kPoolStride == 2 && kVggPoolStride == 2, "pool_kernel's stride");

inline const Network* network_of(int net) { return net == SNERF_LPIPS_ALEX || net == SNERF_LPIPS_VGG16 ? &kNetworks[net] : nullptr; }

// floats: shift[3] scale[3] 0 0 | per convolution: W[k_padded][c_out] (rows k >= k_count are zero), bias[c_out] | lin_0 .. lin_4
struct PackLayout {
    long long weight[kMaxConvs], bias[kMaxConvs], lin[kTaps], total;
};

inline PackLayout pack_layout(const Network& net) {
    PackLayout p = {};
    long long at = 8;
    for (int l = 0; l < net.convs; ++l) {
        p.weight[l] = at;
        at += (long long)k_padded(net.geom[l]) * net.geom[l].c_out;
        p.bias[l] = at;
        at += net.geom[l].c_out;
    }
    for (int l = 0; l < net.convs; ++l) {
        if (net.tap_of[l] < 0) continue;
        p.lin[net.tap_of[l]] = at;
        at += net.geom[l].c_out;
    }
    p.total = at;
    return p;
}

struct Scaling {
    float v[8];
};

__global__ void __launch_bounds__(kBlock) pack_scaling_kernel(Scaling s, float* __restrict__ packed) {
    if (threadIdx.x < 8) packed[threadIdx.x] = s.v[threadIdx.x];
}

// W[k][n] = source[n][c][ky][kx] (torch's OIHW) for k = (ky * kernel + kx) * c_in + c; zero rows up to k_padded
__global__ void __launch_bounds__(kBlock) pack_weight_kernel(const float* __restrict__ source, ConvGeom g, int k_real, long long count,
                                                             float* __restrict__ packed) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        const int k = (int)(i / g.c_out), n = (int)(i - (long long)k * g.c_out);
        float v = 0.0f;
        if (k < k_real) {
            const Tap t = k_tap(g, k);
            v = source[(((long long)n * g.c_in + t.c) * g.kernel + t.ky) * g.kernel + t.kx];
        }
        packed[i] = v;
    }
}

__global__ void __launch_bounds__(kBlock) copy_kernel(const float* __restrict__ source, int count, float* __restrict__ packed) {
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock) packed[i] = source[i];
}

// ------------------------------------------------------------------------------------------------ prepare
__global__ void __launch_bounds__(kBlock) prepare_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ eval,
                                                         const unsigned char* __restrict__ mask, long long pixels,
                                                         const float* __restrict__ packed, float* __restrict__ out) {
    const long long count = 2 * pixels * 3, stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        const long long e = i < pixels * 3 ? i : i - pixels * 3;     // element of the image
        const long long pixel = e / 3;
        const int c = (int)(e - 3 * pixel);
        unsigned char u = gt[e];
        if (i >= pixels * 3 && !(mask && !mask[pixel])) u = eval[e];  // MaskedLPIPS: eval' = mask ? eval : gt
        const float x = (float)u * 2.0f / 255.0f - 1.0f;
        out[i] = (x - packed[c]) / packed[3 + c];
    }
}

// ------------------------------------------------------------------------------------------------ convolution
struct ConvArgs {
    const float* in;       // (2, in_h, in_w, c_in)
    const float* weight;   // [k_padded][c_out]
    const float* bias;     // [c_out]
    float* out;            // (2, out_h, out_w, c_out)
    int in_h, in_w, out_h, out_w;
    int rows;              // 2 * out_h * out_w
};

// One kBM x kBN output tile per workgroup; wave (w >> 1, w & 1) of the 2 x 2 owns 64 pixels x 32 channels = two 32 x 32 MFMA tiles.
// A stage is kSlab = 32 values of k: thread t stages k-column t & 31 of rows (t >> 5) + 8 e (e < 16) of A -- the lanes of a half-wave
// read 32 neighbouring k, which are neighbours in memory inside a tap (NHWC) -- and two 16-byte groups of the weight slab.  The next
// stage's loads are in flight during this stage's 32 MFMAs per wave; out-of-range elements (padding, the row tail, k >= k_real) read
// the tensor's first element and become zeros when they are stored to LDS, so no load is predicated.
// The k sum of an output element: k-pair p of every slab accumulates into chain p % 4, in ascending k; the four chains are added as
// (c0 + c1) + (c2 + c3), then the bias.  Nothing of it depends on the grid.  One instantiation per geometry: it is a compile-time
// constant (the k -> tap divisions cost nothing), and a kernel trace names the geometry (AlexNet's last convolution and VGG-16's
// 256 -> 256 ones are the same kernel).  Where c_in is a multiple of the slab -- every layer but the two first ones -- the 32 values
// of k of a stage lie inside one tap: the tap's (dy, dx) is then decoded once per stage from k0, the same for every thread.
template <int KERNEL, int STRIDE, int PAD, int C_IN, int C_OUT>
__global__ void __launch_bounds__(kBlock, 2) conv_relu_kernel(ConvArgs a) {
    __shared__ float As[2][kSlab][kARow];
    __shared__ __attribute__((aligned(16))) float Bs[2][kSlab][kBRow];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * kBM, n0 = blockIdx.x * kBN;
    constexpr ConvGeom g = {KERNEL, STRIDE, PAD, C_IN, C_OUT, false};
    constexpr int k_real = k_count(g), k_end = k_padded(g);
    constexpr bool slab_in_tap = C_IN % kSlab == 0;
    static_assert(C_OUT % kBN == 0 && (!slab_in_tap || k_real == k_end), "whole column tiles; whole slabs where a slab is one tap");

    // this thread's 16 rows of A: (image, oy, ox) -> the image's offset and the padded source origin, once per kernel
    const int a_k = tid & (kSlab - 1), a_m = tid >> 5;
    int row_image[kRowsPerThread];      // float offset of the row's image in `in`, or -1 for a row past the last pixel
    int row_origin[kRowsPerThread];     // (source origin + pad) of y << 16 | that of x: both in 0 .. 2^15
    const int plane = a.out_h * a.out_w;
#pragma unroll
    for (int e = 0; e < kRowsPerThread; ++e) {
        const int m = m0 + a_m + 8 * e;
        const int image = m / plane, p = m - image * plane, oy = p / a.out_w, ox = p - oy * a.out_w;
        row_image[e] = m < a.rows ? image * (a.in_h * a.in_w * g.c_in) : -1;
        row_origin[e] = ((source_origin(g, oy) + g.pad) << 16) | (source_origin(g, ox) + g.pad);
    }
    const int b_n = (tid & 15) * 4, b_k = tid >> 4;      // weight slab: rows b_k and b_k + 16, four channels from b_n
    const float* const b_src = a.weight + (long long)b_k * g.c_out + n0 + b_n;

    float ra[kRowsPerThread];
    f32x4 rb[2];
    unsigned a_inside = 0;
    auto load_stage = [&](int k0) {
        const int k = k0 + a_k, k_decoded = slab_in_tap ? k0 : k;
        const Tap t = k_tap(g, k_decoded < k_real ? k_decoded : 0);
        const int dy = t.ky - g.pad, dx = t.kx - g.pad, channel = slab_in_tap ? t.c + a_k : t.c;
        const bool k_inside = k < k_real;
        a_inside = 0;
#pragma unroll
        for (int e = 0; e < kRowsPerThread; ++e) {
            const int iy = (row_origin[e] >> 16) + dy, ix = (row_origin[e] & 0xffff) + dx;
            const bool inside = k_inside && row_image[e] >= 0 && in_source(iy, a.in_h) && in_source(ix, a.in_w);
            a_inside |= inside ? 1u << e : 0u;
            ra[e] = a.in[inside ? row_image[e] + (iy * a.in_w + ix) * g.c_in + channel : 0];
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) rb[e] = *reinterpret_cast<const f32x4*>(b_src + (long long)(k0 + 16 * e) * g.c_out);
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int e = 0; e < kRowsPerThread; ++e) As[buf][a_k][a_m + 8 * e] = (a_inside >> e) & 1u ? ra[e] : 0.0f;
#pragma unroll
        for (int e = 0; e < 2; ++e) *reinterpret_cast<f32x4*>(&Bs[buf][b_k + 16 * e][b_n]) = rb[e];
    };

    // MFMA operands: A(m = lane & 31, k = lane >> 5), B(k = lane >> 5, n = lane & 31); result register r of a lane holds
    // row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32, i = lane & 31, h = lane >> 5;
    f32x16 acc[kChains][2];
#pragma unroll
    for (int c = 0; c < kChains; ++c)
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][tm][r] = 0.0f;

    load_stage(0);
    store_stage(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < k_end; k0 += kSlab) {
        const bool more = k0 + kSlab < k_end;
        if (more) load_stage(k0 + kSlab);
        const float* a_rd = &As[buf][h][wm + i];
        const float* b_rd = &Bs[buf][h][wn + i];
#pragma unroll
        for (int p = 0; p < kSlab / 2; ++p) {
            const float b = b_rd[2 * p * kBRow];
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
                acc[p % kChains][tm] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_rd[2 * p * kARow + 32 * tm], b, acc[p % kChains][tm], 0, 0, 0);
        }
        if (more) {
            store_stage(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
    }

    const int n = n0 + wn + i;
    const float bias = a.bias[n];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm + 32 * tm + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m >= a.rows) continue;
            const float sum = (acc[0][tm][r] + acc[1][tm][r]) + (acc[2][tm][r] + acc[3][tm][r]);
            a.out[(long long)m * g.c_out + n] = fmaxf(sum + bias, 0.0f);
        }
}

// ------------------------------------------------------------------------------------------------ max-pool, stride 2
// WINDOW 3: AlexNet's 3 x 3; WINDOW 2: VGG-16's 2 x 2.  Floor mode, no padding: every window lies inside the source (conv_index.h)
template <int WINDOW>
__global__ void __launch_bounds__(kBlock) pool_kernel(const float* __restrict__ in, int in_h, int in_w, int out_h, int out_w, int channels,
                                                      float* __restrict__ out) {
    const long long count = 2LL * out_h * out_w * channels, stride = (long long)gridDim.x * kBlock;
    for (long long idx = (long long)blockIdx.x * kBlock + threadIdx.x; idx < count; idx += stride) {
        const int c = (int)(idx % channels);
        long long rest = idx / channels;
        const int ox = (int)(rest % out_w);
        rest /= out_w;
        const int oy = (int)(rest % out_h), image = (int)(rest / out_h);
        const float* src = in + (((long long)image * in_h + pool_first(oy)) * in_w + pool_first(ox)) * channels + c;
        float v = src[0];
#pragma unroll
        for (int dy = 0; dy < WINDOW; ++dy)
#pragma unroll
            for (int dx = 0; dx < WINDOW; ++dx) v = fmaxf(v, src[((long long)dy * in_w + dx) * channels]);
        out[idx] = v;
    }
}

// ------------------------------------------------------------------------------------------------ layer sums
// One wave per pixel of a tap (grid-stride): lane l takes channels l, l + 64, ...; the channel sums are fp32 (wave_sum leaves the
// same total in every lane), the pixel's value is widened to fp64 and summed per wave in ascending pixel order.
__global__ void __launch_bounds__(kBlock) layer_sums_kernel(const float* __restrict__ features, int pixels, int channels,
                                                            const float* __restrict__ lin, double* __restrict__ partials) {
    __shared__ double lds[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double total = 0.0;
    for (long long p = (long long)blockIdx.x * kWaves + wave; p < pixels; p += (long long)gridDim.x * kWaves) {
        const float* f_gt = features + p * channels;
        const float* f_eval = features + ((long long)pixels + p) * channels;
        float sq_gt = 0.0f, sq_eval = 0.0f;
        for (int c = lane; c < channels; c += 64) {
            sq_gt += f_gt[c] * f_gt[c];
            sq_eval += f_eval[c] * f_eval[c];
        }
        const float norm_gt = sqrtf(snerf::wave_sum(sq_gt)) + 1e-10f, norm_eval = sqrtf(snerf::wave_sum(sq_eval)) + 1e-10f;
        float v = 0.0f;
        for (int c = lane; c < channels; c += 64) {
            const float d = f_gt[c] / norm_gt - f_eval[c] / norm_eval;
            v += lin[c] * (d * d);
        }
        total += (double)snerf::wave_sum(v);
    }
    if (lane == 0) lds[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = lds[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += lds[w];
        partials[blockIdx.x] = s;
    }
}

struct FoldCounts {
    int blocks[kTaps];
};

// ONE workgroup: sums[l] = the layer's partials folded in a fixed order (thread t takes b = t, t + kBlock, ..., then block_sum)
__global__ void __launch_bounds__(kBlock) fold_layers_kernel(const double* __restrict__ partials, FoldCounts counts, double* __restrict__ sums) {
    __shared__ double lds[kWaves];
    for (int l = 0; l < kTaps; ++l) {
        double s = 0.0;
        for (int b = threadIdx.x; b < counts.blocks[l]; b += kBlock) s += partials[l * kMaxPartials + b];
        s = block_sum(s, lds);
        if (threadIdx.x == 0) sums[l] = s;
    }
}

// ------------------------------------------------------------------------------------------------ workspace
inline long long align_up(long long bytes) { return (bytes + 255) / 256 * 256; }

struct Workspace {
    long long input, out[kMaxConvs], pooled[kMaxConvs], partials, total;         // byte offsets
    int out_h[kMaxConvs], out_w[kMaxConvs], in_h[kMaxConvs], in_w[kMaxConvs];    // every convolution's output / (pooled) input extents
    bool fits;                                                                   // every tensor stays below 2^31 floats
};

// AlexNet: every tensor of the chain has a region of its own
inline Workspace plan_alex(int height, int width) {
    Workspace ws = {};
    ws.fits = true;
    auto take = [&](long long floats) {
        if (floats >= (1LL << 31)) ws.fits = false;
        const long long at = ws.total;
        ws.total += align_up(floats * 4);
        return at;
    };
    ws.input = take(2LL * height * width * 3);
    int h = height, w = width;
    for (int l = 0; l < kLayers; ++l) {
        if (kGeom[l].pool_before) {
            h = pool_extent(h);
            w = pool_extent(w);
            ws.pooled[l] = take(2LL * h * w * kGeom[l].c_in);
        }
        ws.in_h[l] = h;
        ws.in_w[l] = w;
        h = conv_extent(h, kGeom[l]);
        w = conv_extent(w, kGeom[l]);
        ws.out_h[l] = h;
        ws.out_w[l] = w;
        ws.out[l] = take(2LL * h * w * kGeom[l].c_out);
    }
    ws.partials = ws.total;
    ws.total += align_up((long long)kTaps * kMaxPartials * 8);
    return ws;
}

// VGG-16: the regions of conv_index.h's vgg_plan (five taps, two ping-pong regions, one pooled region)
static_assert(kVggMaxPartials == kMaxPartials, "one row of partials per tap");
inline Workspace plan_vgg(int height, int width) {
    const VggPlan p = vgg_plan(height, width);
    Workspace ws = {};
    ws.fits = p.fits;
    ws.input = p.input;
    ws.partials = p.partials;
    ws.total = p.total;
    for (int l = 0; l < kVggConvs; ++l) {
        const int target = p.target[l];
        ws.out[l] = target >= 0 ? p.tap[target] : p.ping[target == kVggRegionPing0 ? 0 : 1];
        ws.pooled[l] = p.pooled;
        ws.in_h[l] = p.in_h[l];
        ws.in_w[l] = p.in_w[l];
        ws.out_h[l] = p.out_h[l];
        ws.out_w[l] = p.out_w[l];
    }
    return ws;
}

inline Workspace plan_workspace(int net, int height, int width) { return net == SNERF_LPIPS_VGG16 ? plan_vgg(height, width) : plan_alex(height, width); }

// ------------------------------------------------------------------------------------------------ kernel tables
using ConvKernel = void (*)(ConvArgs);
using PoolKernel = void (*)(const float*, int, int, int, int, int, float*);

template <int KERNEL, int STRIDE, int PAD, int C_IN, int C_OUT>
inline bool is_geometry(const ConvGeom& g) {
    return g.kernel == KERNEL && g.stride == STRIDE && g.pad == PAD && g.c_in == C_IN && g.c_out == C_OUT;
}

// the instantiation for a geometry, or NULL: a network whose table names another one is refused before its first launch
inline ConvKernel conv_kernel_of(const ConvGeom& g) {
#define SNERF_CONV(...) \
    if (is_geometry<__VA_ARGS__>(g)) return conv_relu_kernel<__VA_ARGS__>
    SNERF_CONV(11, 4, 2, 3, 64);       // AlexNet
    SNERF_CONV(5, 1, 2, 64, 192);
    SNERF_CONV(3, 1, 1, 192, 384);
    SNERF_CONV(3, 1, 1, 384, 256);
    SNERF_CONV(3, 1, 1, 256, 256);     // AlexNet's last and VGG-16's conv3_2, conv3_3
    SNERF_CONV(3, 1, 1, 3, 64);        // VGG-16
    SNERF_CONV(3, 1, 1, 64, 64);
    SNERF_CONV(3, 1, 1, 64, 128);
    SNERF_CONV(3, 1, 1, 128, 128);
    SNERF_CONV(3, 1, 1, 128, 256);
    SNERF_CONV(3, 1, 1, 256, 512);
    SNERF_CONV(3, 1, 1, 512, 512);
#undef SNERF_CONV
    return nullptr;
}

inline PoolKernel pool_kernel_of(int window) { return window == 3 ? pool_kernel<3> : window == 2 ? pool_kernel<2> : nullptr; }

}  // namespace

extern "C" long long snerf_lpips_net_packed_floats(int net) {
    const Network* n = network_of(net);
    return n ? pack_layout(*n).total : 0;
}

extern "C" int snerf_lpips_net_pack(int net, const float* const* conv_weights, const float* const* conv_biases,
                                    const float* const* lin_weights, const float* scaling, float* packed, snerf_stream_t stream) {
    const Network* n = network_of(net);
    SNERF_REQUIRE(n, "lpips_pack: network %d is neither SNERF_LPIPS_ALEX nor SNERF_LPIPS_VGG16", net);
    SNERF_REQUIRE(conv_weights && conv_biases && lin_weights && packed, "lpips_pack: NULL pointer");
    for (int l = 0; l < n->convs; ++l) SNERF_REQUIRE(conv_weights[l] && conv_biases[l], "lpips_pack: NULL tensor of layer %d", l);
    for (int t = 0; t < kTaps; ++t) SNERF_REQUIRE(lin_weights[t], "lpips_pack: NULL tensor of layer %d", t);
    const PackLayout layout = pack_layout(*n);
    Scaling s = {{-0.030f, -0.088f, -0.188f, 0.458f, 0.448f, 0.450f, 0.0f, 0.0f}};
    if (scaling)
        for (int j = 0; j < 6; ++j) s.v[j] = scaling[j];
    for (int c = 0; c < 3; ++c) SNERF_REQUIRE(s.v[3 + c] != 0.0f, "lpips_pack: scale[%d] is zero", c);
    hipStream_t hs = (hipStream_t)stream;
    hipLaunchKernelGGL(pack_scaling_kernel, dim3(1), dim3(kBlock), 0, hs, s, packed);
    for (int l = 0; l < n->convs; ++l) {
        const ConvGeom g = n->geom[l];
        const long long count = (long long)k_padded(g) * g.c_out;
        hipLaunchKernelGGL(pack_weight_kernel, dim3(snerf::stride_grid(count, kBlock)), dim3(kBlock), 0, hs, conv_weights[l], g, k_count(g),
                           count, packed + layout.weight[l]);
        hipLaunchKernelGGL(copy_kernel, dim3(1), dim3(kBlock), 0, hs, conv_biases[l], g.c_out, packed + layout.bias[l]);
        if (n->tap_of[l] >= 0)
            hipLaunchKernelGGL(copy_kernel, dim3(1), dim3(kBlock), 0, hs, lin_weights[n->tap_of[l]], g.c_out, packed + layout.lin[n->tap_of[l]]);
    }
    return snerf::check_launch("lpips_pack");
}

extern "C" long long snerf_lpips_net_workspace_bytes(int net, int height, int width) {
    const Network* n = network_of(net);
    if (!n || height < n->min_extent || width < n->min_extent) return 0;
    const Workspace ws = plan_workspace(net, height, width);
    return ws.fits ? ws.total : 0;
}

extern "C" int snerf_lpips_net_tap_shape(int net, int height, int width, int layer, int* tap_height, int* tap_width, int* channels) {
    const Network* n = network_of(net);
    SNERF_REQUIRE(n, "lpips_tap_shape: network %d is neither SNERF_LPIPS_ALEX nor SNERF_LPIPS_VGG16", net);
    SNERF_REQUIRE(tap_height && tap_width && channels, "lpips_tap_shape: NULL pointer");
    SNERF_REQUIRE(layer >= 0 && layer < kTaps, "lpips_tap_shape: layer %d outside 0..%d", layer, kTaps - 1);
    SNERF_REQUIRE(height >= n->min_extent && width >= n->min_extent, "lpips_tap_shape: a %d x %d image is smaller than the network's %d x %d",
                  height, width, n->min_extent, n->min_extent);
    if (net == SNERF_LPIPS_VGG16) {
        *tap_height = vgg_tap_extent(height, layer);
        *tap_width = vgg_tap_extent(width, layer);
        *channels = kVggGeom[kVggTapConv[layer]].c_out;
    } else {
        *tap_height = tap_extent(height, layer);
        *tap_width = tap_extent(width, layer);
        *channels = kGeom[layer].c_out;
    }
    return SNERF_OK;
}

extern "C" int snerf_lpips_net_sums(int net, const unsigned char* gt, const unsigned char* eval, const unsigned char* mask, int height,
                                    int width, const float* packed, double* sums, float* const* taps, void* workspace,
                                    snerf_stream_t stream) {
    const Network* n = network_of(net);
    SNERF_REQUIRE(n, "lpips_sums: network %d is neither SNERF_LPIPS_ALEX nor SNERF_LPIPS_VGG16", net);
    SNERF_REQUIRE(gt && eval && packed && sums && workspace, "lpips_sums: NULL pointer");
    SNERF_REQUIRE(height >= n->min_extent && width >= n->min_extent, "lpips_sums: a %d x %d image is smaller than the network's %d x %d",
                  height, width, n->min_extent, n->min_extent);
    const Workspace ws = plan_workspace(net, height, width);
    SNERF_REQUIRE(ws.fits && height <= 16384 && width <= 16384, "lpips_sums: a %d x %d image exceeds the 32-bit activation index", height, width);
    ConvKernel conv[kMaxConvs];
    for (int l = 0; l < n->convs; ++l) {
        conv[l] = conv_kernel_of(n->geom[l]);
        SNERF_REQUIRE(conv[l], "lpips_sums: no convolution kernel for layer %d of %s", l, n->name);
        SNERF_REQUIRE((2LL * ws.out_h[l] * ws.out_w[l] + kBM - 1) / kBM <= 65535, "lpips_sums: a %d x %d image exceeds the grid", height, width);
    }
    const PoolKernel pool = pool_kernel_of(n->pool_window);
    SNERF_REQUIRE(pool, "lpips_sums: no pool kernel for %s", n->name);
    const PackLayout layout = pack_layout(*n);
    hipStream_t hs = (hipStream_t)stream;
    char* base = (char*)workspace;
    float* input = (float*)(base + ws.input);
    double* partials = (double*)(base + ws.partials);

    const long long pixels = (long long)height * width;
    hipLaunchKernelGGL(prepare_kernel, dim3(snerf::stride_grid(6 * pixels, kBlock)), dim3(kBlock), 0, hs, gt, eval, mask, pixels, packed, input);
    const float* previous = input;
    FoldCounts counts = {};
    for (int l = 0; l < n->convs; ++l) {
        const ConvGeom g = n->geom[l];
        const int tap = n->tap_of[l];
        if (g.pool_before) {
            float* pooled = (float*)(base + ws.pooled[l]);
            const long long count = 2LL * ws.in_h[l] * ws.in_w[l] * g.c_in;
            hipLaunchKernelGGL(pool, dim3(snerf::stride_grid(count, kBlock)), dim3(kBlock), 0, hs, previous, ws.out_h[l - 1], ws.out_w[l - 1],
                               ws.in_h[l], ws.in_w[l], g.c_in, pooled);
            previous = pooled;
        }
        float* out = tap >= 0 && taps && taps[tap] ? taps[tap] : (float*)(base + ws.out[l]);
        ConvArgs a;
        a.in = previous;
        a.weight = packed + layout.weight[l];
        a.bias = packed + layout.bias[l];
        a.out = out;
        a.in_h = ws.in_h[l];
        a.in_w = ws.in_w[l];
        a.out_h = ws.out_h[l];
        a.out_w = ws.out_w[l];
        a.rows = 2 * a.out_h * a.out_w;
        const dim3 grid(g.c_out / kBN, (a.rows + kBM - 1) / kBM);
        hipLaunchKernelGGL(conv[l], grid, dim3(kBlock), 0, hs, a);
        if (tap >= 0) {
            const int tap_pixels = a.out_h * a.out_w;
            int blocks = (tap_pixels + kWaves - 1) / kWaves;
            if (blocks > kMaxPartials) blocks = kMaxPartials;
            counts.blocks[tap] = blocks;
            hipLaunchKernelGGL(layer_sums_kernel, dim3(blocks), dim3(kBlock), 0, hs, (const float*)out, tap_pixels, g.c_out,
                               packed + layout.lin[tap], partials + tap * kMaxPartials);
        }
        previous = out;
    }
    hipLaunchKernelGGL(fold_layers_kernel, dim3(1), dim3(kBlock), 0, hs, (const double*)partials, counts, sums);
    return snerf::check_launch("lpips_sums");
}

// the AlexNet entry points: the selector fixed
extern "C" long long snerf_lpips_packed_floats(void) { return snerf_lpips_net_packed_floats(SNERF_LPIPS_ALEX); }

extern "C" int snerf_lpips_pack(const float* const* conv_weights, const float* const* conv_biases, const float* const* lin_weights,
                                const float* scaling, float* packed, snerf_stream_t stream) {
    return snerf_lpips_net_pack(SNERF_LPIPS_ALEX, conv_weights, conv_biases, lin_weights, scaling, packed, stream);
}

extern "C" long long snerf_lpips_workspace_bytes(int height, int width) { return snerf_lpips_net_workspace_bytes(SNERF_LPIPS_ALEX, height, width); }

extern "C" int snerf_lpips_tap_shape(int height, int width, int layer, int* tap_height, int* tap_width, int* channels) {
    return snerf_lpips_net_tap_shape(SNERF_LPIPS_ALEX, height, width, layer, tap_height, tap_width, channels);
}

extern "C" int snerf_lpips_sums(const unsigned char* gt, const unsigned char* eval, const unsigned char* mask, int height, int width,
                                const float* packed, double* sums, float* const* taps, void* workspace, snerf_stream_t stream) {
    return snerf_lpips_net_sums(SNERF_LPIPS_ALEX, gt, eval, mask, height, width, packed, sums, taps, workspace, stream);
}
