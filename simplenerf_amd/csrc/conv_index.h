// Index arithmetic of the LPIPS convolutions (csrc/lpips.hip), free of device code so that a host program can walk it under
// sanitizers (tests/native/conv_index_test.cpp, conv_index_vgg_test.cpp): the five AlexNet layers' geometry, output extents, the GEMM
// k index <-> (tap row, tap column, channel), the source coordinate of an (output pixel, tap) with its padding predicate, and the
// 3 x 3 stride-2 pool; below them VGG-16's thirteen layers, its 2 x 2 stride-2 pool, its tap extents and its workspace plan.
//
// Activations are NHWC.  A convolution is the product  out[m][n] = sum_k A[m][k] W[k][n]  with m = (image, oy, ox) row-major,
// n = output channel and k = (ky * kernel + kx) * c_in + c: the channels of one tap are neighbours in k as they are in memory.
#pragma once

#ifdef __HIPCC__
#define SNERF_HD __host__ __device__ constexpr
#else
#define SNERF_HD constexpr
#endif

namespace snerf {
namespace conv_index {

struct ConvGeom {
    int kernel, stride, pad, c_in, c_out;
    bool pool_before;   // a 3 x 3 stride-2 max-pool (no padding, floor mode) runs on the layer's input first
};

constexpr int kLayers = 5;
constexpr int kSlab = 32;   // k values per GEMM stage: every layer's K is padded to a multiple of it (zero weights)
// torchvision's AlexNet `features`, taps after each ReLU: conv 0, (pool 2) conv 3, (pool 5) conv 6, conv 8, conv 10
constexpr ConvGeom kGeom[kLayers] = {
    {11, 4, 2, 3, 64, false}, {5, 1, 2, 64, 192, true}, {3, 1, 1, 192, 384, true}, {3, 1, 1, 384, 256, false}, {3, 1, 1, 256, 256, false}};
constexpr int kPoolWindow = 3, kPoolStride = 2;
constexpr int kMinExtent = 31;   // the smallest side the network accepts: relu1 7 -> pool 3 -> pool 1

SNERF_HD int conv_extent(int in, const ConvGeom& g) { return (in + 2 * g.pad - g.kernel) / g.stride + 1; }
SNERF_HD int pool_extent(int in) { return (in - kPoolWindow) / kPoolStride + 1; }
// extent of layer `layer`'s output (its tap) along a side of `in` image pixels; 0 when the image is too small
SNERF_HD int tap_extent(int in, int layer) {
    if (in < kMinExtent) return 0;
    for (int l = 0; l <= layer; ++l) {
        if (kGeom[l].pool_before) in = pool_extent(in);
        in = conv_extent(in, kGeom[l]);
    }
    return in;
}

SNERF_HD int k_count(const ConvGeom& g) { return g.kernel * g.kernel * g.c_in; }
SNERF_HD int k_padded(const ConvGeom& g) { return (k_count(g) + kSlab - 1) / kSlab * kSlab; }

struct Tap {
    int ky, kx, c;
};
SNERF_HD int k_index(const ConvGeom& g, int ky, int kx, int c) { return (ky * g.kernel + kx) * g.c_in + c; }
SNERF_HD Tap k_tap(const ConvGeom& g, int k) {   // 0 <= k < k_count(g)
    const int t = k / g.c_in;
    return Tap{t / g.kernel, t % g.kernel, k % g.c_in};
}

// first source coordinate (tap 0) of output coordinate o: negative inside the padding
SNERF_HD int source_origin(const ConvGeom& g, int o) { return o * g.stride - g.pad; }
// tap `t` of output `o` reads source coordinate source_origin + t; it is padding (a zero) unless 0 <= coordinate < extent
SNERF_HD bool in_source(int coordinate, int extent) { return coordinate >= 0 && coordinate < extent; }

// the pool window of output o covers source pool_first(o) .. pool_first(o) + kPoolWindow - 1, all inside the source (floor mode)
SNERF_HD int pool_first(int o) { return o * kPoolStride; }

// ---------------------------------------------------------------------------------------------------- VGG-16
// torchvision's vgg16 `features`: thirteen 3 x 3 stride-1 pad-1 convolutions (indices 0 2 | 5 7 | 10 12 14 | 17 19 21 | 24 26 28),
// each followed by a ReLU, with a 2 x 2 stride-2 max-pool (no padding, floor mode) in front of convolutions 2, 4, 7 and 10 (the
// pools at indices 4, 9, 16, 23; the one at 30 is not used).  `pool_before` of this table means THAT pool.
constexpr int kVggConvs = 13, kVggTaps = 5;
constexpr ConvGeom kVggGeom[kVggConvs] = {
    {3, 1, 1, 3, 64, false},    {3, 1, 1, 64, 64, false},   {3, 1, 1, 64, 128, true},   {3, 1, 1, 128, 128, false}, {3, 1, 1, 128, 256, true},
    {3, 1, 1, 256, 256, false}, {3, 1, 1, 256, 256, false}, {3, 1, 1, 256, 512, true},  {3, 1, 1, 512, 512, false}, {3, 1, 1, 512, 512, false},
    {3, 1, 1, 512, 512, true},  {3, 1, 1, 512, 512, false}, {3, 1, 1, 512, 512, false}};
// the LPIPS tap a convolution's ReLU feeds (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3), or -1
constexpr int kVggTapOf[kVggConvs] = {-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4};
constexpr int kVggTapConv[kVggTaps] = {1, 3, 6, 9, 12};
constexpr int kVggPoolWindow = 2, kVggPoolStride = 2;
constexpr int kVggMinExtent = 16;   // the smallest side: 16 -> 8 -> 4 -> 2 -> 1

SNERF_HD int vgg_pool_extent(int in) { return (in - kVggPoolWindow) / kVggPoolStride + 1; }
// the window of output o covers source vgg_pool_first(o) .. + kVggPoolWindow - 1, all inside the source (floor mode)
SNERF_HD int vgg_pool_first(int o) { return o * kVggPoolStride; }
// extent of convolution `conv`'s output along a side of `in` image pixels; 0 when the image is too small
SNERF_HD int vgg_conv_output_extent(int in, int conv) {
    if (in < kVggMinExtent) return 0;
    for (int l = 0; l <= conv; ++l) {
        if (kVggGeom[l].pool_before) in = vgg_pool_extent(in);
        in = conv_extent(in, kVggGeom[l]);
    }
    return in;
}
SNERF_HD int vgg_tap_extent(int in, int tap) { return vgg_conv_output_extent(in, kVggTapConv[tap]); }

// Workspace of one pass over a height x width pair, as byte offsets of disjoint regions.  Every activation is fp32 NHWC over BOTH
// images.  The five taps keep a region each (the layer sums read them after the chain has moved on, and a pool reads the tap in
// front of it); a convolution that feeds no tap writes ping[0] when its input is the image or a pooled tensor and ping[1] when its
// input is ping[0] (conv3_2, conv4_2, conv5_2), so no convolution reads the region it writes; one pooled region serves all four
// pools (the convolution that read it has finished before the next pool writes it: one stream, in order).
struct VggPlan {
    long long input, tap[kVggTaps], ping[2], pooled, partials, total;                 // byte offsets, 256-byte aligned
    long long input_bytes, tap_bytes[kVggTaps], ping_bytes[2], pooled_bytes, partials_bytes;
    int in_h[kVggConvs], in_w[kVggConvs], out_h[kVggConvs], out_w[kVggConvs];         // every convolution's (pooled) input and output
    int source[kVggConvs], target[kVggConvs];     // region read / written by a convolution: kVggRegion* or a tap number
    bool fits;                                    // every tensor stays below 2^31 floats
};
constexpr int kVggRegionInput = -1, kVggRegionPooled = -2, kVggRegionPing0 = -3, kVggRegionPing1 = -4;
constexpr int kVggMaxPartials = 1024;   // fp64 partial sums of a tap's reduction, one row of them per tap

inline VggPlan vgg_plan(int height, int width) {
    VggPlan p = {};
    p.fits = true;
    long long ping_floats[2] = {0, 0}, pooled_floats = 0, tap_floats[kVggTaps] = {};
    auto note = [&](long long floats, long long& most) {
        if (floats >= (1LL << 31)) p.fits = false;
        if (floats > most) most = floats;
    };
    int h = height, w = width, previous = kVggRegionInput;
    for (int l = 0; l < kVggConvs; ++l) {
        const ConvGeom g = kVggGeom[l];
        if (g.pool_before) {
            h = vgg_pool_extent(h);
            w = vgg_pool_extent(w);
            note(2LL * h * w * g.c_in, pooled_floats);
            previous = kVggRegionPooled;
        }
        p.in_h[l] = h;
        p.in_w[l] = w;
        h = conv_extent(h, g);
        w = conv_extent(w, g);
        p.out_h[l] = h;
        p.out_w[l] = w;
        p.source[l] = previous;
        const long long floats = 2LL * h * w * g.c_out;
        if (kVggTapOf[l] >= 0) {
            p.target[l] = kVggTapOf[l];
            note(floats, tap_floats[kVggTapOf[l]]);
        } else {
            p.target[l] = previous == kVggRegionPing0 ? kVggRegionPing1 : kVggRegionPing0;
            note(floats, ping_floats[p.target[l] == kVggRegionPing0 ? 0 : 1]);
        }
        previous = p.target[l];
    }
    auto take = [&](long long bytes, long long& size) {
        const long long at = p.total;
        size = bytes;
        p.total += (bytes + 255) / 256 * 256;
        return at;
    };
    long long input_floats = 0;
    note(2LL * height * width * 3, input_floats);
    p.input = take(input_floats * 4, p.input_bytes);
    for (int t = 0; t < kVggTaps; ++t) p.tap[t] = take(tap_floats[t] * 4, p.tap_bytes[t]);
    for (int i = 0; i < 2; ++i) p.ping[i] = take(ping_floats[i] * 4, p.ping_bytes[i]);
    p.pooled = take(pooled_floats * 4, p.pooled_bytes);
    p.partials = take((long long)kVggTaps * kVggMaxPartials * 8, p.partials_bytes);
    return p;
}

}  // namespace conv_index
}  // namespace snerf
