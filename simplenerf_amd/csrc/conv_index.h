// Index arithmetic of the LPIPS convolutions (csrc/lpips.hip), free of device code so that a host program can walk it under
// sanitizers (tests/native/conv_index_test.cpp): the five AlexNet layers' geometry, output extents, the GEMM k index <-> (tap row,
// tap column, channel), the source coordinate of an (output pixel, tap) with its padding predicate, and the 3 x 3 stride-2 pool.
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

}  // namespace conv_index
}  // namespace snerf
