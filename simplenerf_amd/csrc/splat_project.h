// The projection of the splat (the reference's Warper.compute_transformed_points and the flow round trip of forward_warp) and the
// maximum fold that follows it, shared by the visibility masks (visibility_mask.hip) and the Warper (warp.hip): both launch the SAME
// kernel, so a view projected by either returns the same bits.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "splat_cells.h"

namespace snerf {
namespace splat {

constexpr int kProjectBlock = 256;
constexpr int kProjectWaves = kProjectBlock / 64;
constexpr int kMaxPartials = 1024;   // workgroups per view of a projection
constexpr int kCamera = 30;          // doubles per training view: inv(K_train) 3x3 | rows 0..2 of E_test inv(E_train) 3x4 | K_test 3x3

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// Maximum of `v` over the workgroup, valid in thread 0 (fmax: a NaN is ignored).  `lds` holds kProjectWaves values; reusable after
// the call.
__device__ __forceinline__ double block_max(double v, double* lds) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = lds[0];
#pragma unroll
    for (int k = 1; k < kProjectWaves; ++k) m = fmax(m, lds[k]);
    return m;
}

struct Camera {
    double ki[9], tr[12], k2[9];
};

__device__ __forceinline__ Camera load_camera(const double* __restrict__ cam) {
    Camera c;
#pragma unroll
    for (int j = 0; j < 9; ++j) c.ki[j] = cam[j];
#pragma unroll
    for (int j = 0; j < 12; ++j) c.tr[j] = cam[9 + j];
#pragma unroll
    for (int j = 0; j < 9; ++j) c.k2[j] = cam[21 + j];
    return c;
}

// Source pixel (x, y) of depth d: Warper.compute_transformed_points in its own order (inv(K_train) (x, y, 1), times the depth, the
// 4x4 transform, K_test), the flow (u, v) = q / q2 - grid, and the padded position through the reference's round trip
// (flow + grid) + 1.
__device__ __forceinline__ void project_source(const Camera& c, double x, double y, double d, double& X, double& Y, double& Z, double& u,
                                               double& v) {
    double p[3], t[3], q[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = d * (c.ki[3 * j] * x + c.ki[3 * j + 1] * y + c.ki[3 * j + 2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = c.tr[4 * j] * p[0] + c.tr[4 * j + 1] * p[1] + c.tr[4 * j + 2] * p[2] + c.tr[4 * j + 3];
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] = c.k2[3 * j] * t[0] + c.k2[3 * j + 1] * t[1] + c.k2[3 * j + 2] * t[2];
    u = q[0] / q[2] - x;
    v = q[1] / q[2] - y;
    X = (u + x) + 1.0;
    Y = (v + y) + 1.0;
    Z = q[2];
}

// grid (blocks, views): every source pixel of every view.  points = planes X, Y, Z per view; keys = key of the view's first list +
// the source's list (the discard key where `mask`, (views, h, w) bytes or NULL, drops it); flow = (views, h, w, 2) or NULL: (u, v)
// of every source; partial = (max L, max d) of the workgroup's pixels, masked ones included.  The ONE projection of the masks and
// of the Warper: a rule changed here changes for both.
static __global__ void __launch_bounds__(kProjectBlock) project_kernel(const float* __restrict__ depths, const double* __restrict__ cameras,
                                                                       const unsigned char* __restrict__ mask, int height, int width,
                                                                       double* __restrict__ points, int* __restrict__ keys,
                                                                       double* __restrict__ flow, double* __restrict__ partials) {
    __shared__ double lds[kProjectWaves];
    const int view = blockIdx.y;
    const long long n = (long long)height * width;
    const Camera cam = load_camera(cameras + (long long)view * kCamera);
    const float* depth = depths + view * n;
    double* px = points + (long long)view * 3 * n;
    double* py = px + n;
    double* pz = py + n;
    const int key_base = view * keys_per_view(height, width);
    double max_l = 0.0, max_d = -INFINITY;
    const long long stride = (long long)gridDim.x * kProjectBlock;
    for (long long i = (long long)blockIdx.x * kProjectBlock + threadIdx.x; i < n; i += stride) {
        const int yi = (int)(i / width), xi = (int)(i - (long long)yi * width);
        const double x = (double)xi, y = (double)yi, d = (double)depth[i];
        double X, Y, Z, u, v;
        project_source(cam, x, y, d, X, Y, Z, u, v);
        px[i] = X;
        py[i] = Y;
        pz[i] = Z;
        if (flow) {
            flow[2 * (view * n + i)] = u;
            flow[2 * (view * n + i) + 1] = v;
        }
        const bool dropped = mask && mask[view * n + i] == 0;
        keys[view * n + i] = key_base + (dropped ? cell_keys(height, width) : source_key(X, Y, Z, height, width));
        max_l = fmax(max_l, log_depth(Z));
        max_d = fmax(max_d, d);
    }
    max_l = block_max(max_l, lds);
    max_d = block_max(max_d, lds);
    if (threadIdx.x == 0) {
        double* out = partials + ((long long)view * gridDim.x + blockIdx.x) * 2;
        out[0] = max_l;
        out[1] = max_d;
    }
}

// grid (views), ONE workgroup per view: stats[view] = (max L, max d) over the view's partials, thread t taking b = t, t + block, ...
static __global__ void __launch_bounds__(kProjectBlock) fold_max_kernel(const double* __restrict__ partials, int num_partials,
                                                                        double* __restrict__ stats) {
    __shared__ double lds[kProjectWaves];
    const double* in = partials + (long long)blockIdx.x * num_partials * 2;
    double max_l = 0.0, max_d = -INFINITY;
    for (int b = threadIdx.x; b < num_partials; b += kProjectBlock) {
        max_l = fmax(max_l, in[2 * b]);
        max_d = fmax(max_d, in[2 * b + 1]);
    }
    max_l = block_max(max_l, lds);
    max_d = block_max(max_d, lds);
    if (threadIdx.x == 0) {
        stats[2 * blockIdx.x] = max_l;
        stats[2 * blockIdx.x + 1] = max_d;
    }
}

inline int project_blocks(long long pixels) {
    long long blocks = (pixels + kProjectBlock - 1) / kProjectBlock;
    if (blocks > kMaxPartials) blocks = kMaxPartials;
    return blocks < 1 ? 1 : (int)blocks;
}

// views * height * width sources and views * keys_per_view keys must both fit int32 (keys, list starts)
inline bool fits(int views, int height, int width) {
    if (views < 1 || height < 1 || width < 1) return false;
    const long long keys = (long long)views * ((long long)(height + 1) * (width + 1) + 1);
    return keys < 2147483647LL && (long long)views <= 65535;
}

}  // namespace splat
}  // namespace snerf
