// Q2: the visibility masks of the masked frame metrics (the reference's src/qa/00_Common/src/mask_generators: Warper.forward_warp,
// MaskComputer.compute_mask and the scripts' "visible in at least two training views").  A training view's depth is splatted into the
// test view -- every source pixel adds a proximity x depth weight to the (up to) four cells around its projected position -- and a
// test pixel is visible from that view where something landed and the splatted depth agrees with the test depth.
//
// The reference scatters (numpy.add.at).  Here every reduction must return the same bits on every call, which excludes float atomics,
// so the scatter is turned round: project stores each source's position and the key of its floor cell, the caller sorts the keys
// (stable: every list keeps ascending source order), list_starts finds where each key's list begins, and gather gives every
// destination pixel one thread that walks the at most four lists that can reach it (splat_cells.h) in a fixed order.  All arithmetic
// is fp64 (the fp32 depths are widened on load, as numpy's promotion does); this file holds no fp32 arithmetic.  Bound: project and
// gather by fp64 divide / exp / log rate and the 28 bytes per source they move, the other two by memory latency.
#include <cmath>

#include "snerf_common.h"
#include "splat_cells.h"

namespace {

using namespace snerf::splat;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxPartials = 1024;   // workgroups per view of the projection
constexpr int kCamera = 30;          // doubles per training view: inv(K_train) 3x3 | rows 0..2 of E_test inv(E_train) 3x4 | K_test 3x3

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// Maximum of `v` over the workgroup, valid in thread 0 (fmax: a NaN is ignored).  `lds` holds kWaves values; reusable after the call.
__device__ __forceinline__ double block_max(double v, double* lds) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = lds[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) m = fmax(m, lds[k]);
    return m;
}

// ------------------------------------------------------------------------------------------------ project
// grid (blocks, views).  Per source pixel: Warper.compute_transformed_points in its own order (inv(K_train) (x, y, 1), times the
// depth, the 4x4 transform, K_test), the position through the reference's flow round trip ((q / q2 - grid) + grid) + 1, its key.
// partial = (max L, max d_train) of the workgroup's pixels.
__global__ void __launch_bounds__(kBlock) project_kernel(const float* __restrict__ depth_train, const double* __restrict__ cameras, int height,
                                                         int width, double* __restrict__ points, int* __restrict__ keys,
                                                         double* __restrict__ partials) {
    __shared__ double lds[kWaves];
    const int view = blockIdx.y;
    const long long n = (long long)height * width;
    const double* cam = cameras + (long long)view * kCamera;
    double ki[9], tr[12], k2[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) ki[j] = cam[j];
#pragma unroll
    for (int j = 0; j < 12; ++j) tr[j] = cam[9 + j];
#pragma unroll
    for (int j = 0; j < 9; ++j) k2[j] = cam[21 + j];
    const float* depth = depth_train + view * n;
    double* px = points + (long long)view * 3 * n;
    double* py = px + n;
    double* pz = py + n;
    const int key_base = view * keys_per_view(height, width);
    double max_l = 0.0, max_d = -INFINITY;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int yi = (int)(i / width), xi = (int)(i - (long long)yi * width);
        const double x = (double)xi, y = (double)yi, d = (double)depth[i];
        double p[3], t[3], q[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) p[j] = d * (ki[3 * j] * x + ki[3 * j + 1] * y + ki[3 * j + 2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = tr[4 * j] * p[0] + tr[4 * j + 1] * p[1] + tr[4 * j + 2] * p[2] + tr[4 * j + 3];
#pragma unroll
        for (int j = 0; j < 3; ++j) q[j] = k2[3 * j] * t[0] + k2[3 * j + 1] * t[1] + k2[3 * j + 2] * t[2];
        const double X = ((q[0] / q[2] - x) + x) + 1.0, Y = ((q[1] / q[2] - y) + y) + 1.0, Z = q[2];
        px[i] = X;
        py[i] = Y;
        pz[i] = Z;
        keys[view * n + i] = key_base + source_key(X, Y, Z, height, width);
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

// grid (views), ONE workgroup per view: stats[view] = (max L, max d_train) over the view's partials, thread t taking b = t, t + kBlock, ...
__global__ void __launch_bounds__(kBlock) fold_max_kernel(const double* __restrict__ partials, int num_partials, double* __restrict__ stats) {
    __shared__ double lds[kWaves];
    const double* in = partials + (long long)blockIdx.x * num_partials * 2;
    double max_l = 0.0, max_d = -INFINITY;
    for (int b = threadIdx.x; b < num_partials; b += kBlock) {
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

// ------------------------------------------------------------------------------------------------ list starts
// starts[k] = first index with sorted_keys[i] >= k (lower bound), k = 0 .. num_keys: list k is sorted positions starts[k] .. starts[k + 1].
__global__ void __launch_bounds__(kBlock) list_starts_kernel(const int* __restrict__ sorted_keys, long long count, long long num_keys,
                                                             int* __restrict__ starts) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k <= num_keys; k += stride) {
        long long lo = 0, hi = count;
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (sorted_keys[mid] < k) lo = mid + 1; else hi = mid;
        }
        starts[k] = (int)lo;
    }
}

// ------------------------------------------------------------------------------------------------ gather
// One thread per (view, destination pixel): the padded cell (y + 1, x + 1) sums what the sources of its four lists add to it, list by
// list, each list in ascending source order, each source's corners in the order nw, sw, ne, se; then the depth test.
__global__ void __launch_bounds__(kBlock) gather_kernel(const double* __restrict__ points, const long long* __restrict__ order,
                                                        const int* __restrict__ starts, const double* __restrict__ stats,
                                                        const float* __restrict__ depth_test, double depth_error_threshold, int views,
                                                        int height, int width, unsigned char* __restrict__ mask_views,
                                                        double* __restrict__ warped_depth, double* __restrict__ weight_sum) {
    const long long n = (long long)height * width, total = n * views;
    const int per_view = keys_per_view(height, width);
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int view = (int)(i / n);
        const long long pixel = i - view * n;
        const int y = (int)(pixel / width), x = (int)(pixel - (long long)y * width);
        const double max_l = stats[2 * view], max_d = stats[2 * view + 1];
        const double* px = points + (long long)view * 3 * n;
        const double* py = px + n;
        const double* pz = py + n;
        double zw = 0.0, ws = 0.0;
        if (max_l > 0.0) {   // (max L = 0: every weight is 0 / 0 in the reference; nothing is added here)
            int lists[4];
            const int num_lists = lists_of(y + 1, x + 1, width, lists);
            for (int l = 0; l < num_lists; ++l) {
                const long long key = (long long)view * per_view + lists[l];
                const int first = starts[key], last = starts[key + 1];
                for (int s = first; s < last; ++s) {
                    const long long source = order[s] - view * n;
                    if (source < 0 || source >= n) continue;   // (not an index of this view: an `order` that is no sort of `keys`)
                    const double Z = pz[source];
                    add_source(px[source], py[source], Z, depth_divisor(Z, max_l), y + 1, x + 1, height, width, zw, ws);
                }
            }
        }
        const bool warped = ws > 0.0;
        const double depth = warped ? zw / ws : 0.0;
        mask_views[i] = (warped && fabs(depth - (double)depth_test[pixel]) < depth_error_threshold * max_d) ? 1 : 0;
        if (warped_depth) warped_depth[i] = depth;
        if (weight_sum) weight_sum[i] = ws;
    }
}

// ------------------------------------------------------------------------------------------------ combine
__global__ void __launch_bounds__(kBlock) combine_kernel(const unsigned char* __restrict__ mask_views, int views, long long pixels,
                                                         int min_views, unsigned char* __restrict__ mask) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < pixels; i += stride) {
        int seen = 0;
        for (int v = 0; v < views; ++v) seen += mask_views[v * pixels + i] ? 1 : 0;
        mask[i] = seen >= min_views ? 1 : 0;
    }
}

inline int project_blocks(long long pixels) {
    long long blocks = (pixels + kBlock - 1) / kBlock;
    if (blocks > kMaxPartials) blocks = kMaxPartials;
    return blocks < 1 ? 1 : (int)blocks;
}

// views * height * width sources and views * keys_per_view keys must both fit int32 (keys, list starts)
inline bool fits(int views, int height, int width) {
    if (views < 1 || height < 1 || width < 1) return false;
    const long long keys = (long long)views * ((long long)(height + 1) * (width + 1) + 1);
    return keys < 2147483647LL && (long long)views <= 65535;
}

}  // namespace

extern "C" long long snerf_visibility_mask_workspace_bytes(int views, int height, int width) {
    if (!fits(views, height, width)) return 0;
    return (long long)views * kMaxPartials * 2 * 8;
}

extern "C" int snerf_visibility_mask_project(const float* depth_train, const double* cameras, int views, int height, int width,
                                             double* points, int* keys, double* stats, void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(depth_train && cameras && points && keys && stats && workspace, "visibility_mask_project: NULL pointer");
    SNERF_REQUIRE(fits(views, height, width), "visibility_mask_project: %d views of %d x %d are empty or exceed int32 keys", views, height, width);
    const int blocks = project_blocks((long long)height * width);
    double* partials = (double*)workspace;
    hipLaunchKernelGGL(project_kernel, dim3(blocks, views), dim3(kBlock), 0, (hipStream_t)stream, depth_train, cameras, height, width,
                       points, keys, partials);
    hipLaunchKernelGGL(fold_max_kernel, dim3(views), dim3(kBlock), 0, (hipStream_t)stream, (const double*)partials, blocks, stats);
    return snerf::check_launch("visibility_mask_project");
}

extern "C" int snerf_visibility_mask_list_starts(const int* sorted_keys, int views, int height, int width, int* starts,
                                                 snerf_stream_t stream) {
    SNERF_REQUIRE(sorted_keys && starts, "visibility_mask_list_starts: NULL pointer");
    SNERF_REQUIRE(fits(views, height, width), "visibility_mask_list_starts: %d views of %d x %d are empty or exceed int32 keys", views, height, width);
    const long long count = (long long)views * height * width, num_keys = (long long)views * keys_per_view(height, width);
    hipLaunchKernelGGL(list_starts_kernel, dim3(snerf::stride_grid(num_keys + 1, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       sorted_keys, count, num_keys, starts);
    return snerf::check_launch("visibility_mask_list_starts");
}

extern "C" int snerf_visibility_mask_gather(const double* points, const long long* order, const int* starts, const double* stats,
                                            const float* depth_test, double depth_error_threshold, int views, int height, int width,
                                            unsigned char* mask_views, double* warped_depth, double* weight_sum, snerf_stream_t stream) {
    SNERF_REQUIRE(points && order && starts && stats && depth_test && mask_views, "visibility_mask_gather: NULL pointer");
    SNERF_REQUIRE(fits(views, height, width), "visibility_mask_gather: %d views of %d x %d are empty or exceed int32 keys", views, height, width);
    const long long total = (long long)views * height * width;
    hipLaunchKernelGGL(gather_kernel, dim3(snerf::stride_grid(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, points, order, starts,
                       stats, depth_test, depth_error_threshold, views, height, width, mask_views, warped_depth, weight_sum);
    return snerf::check_launch("visibility_mask_gather");
}

extern "C" int snerf_visibility_mask_combine(const unsigned char* mask_views, int views, int height, int width, int min_views,
                                             unsigned char* mask, snerf_stream_t stream) {
    SNERF_REQUIRE(mask_views && mask, "visibility_mask_combine: NULL pointer");
    SNERF_REQUIRE(fits(views, height, width), "visibility_mask_combine: %d views of %d x %d are empty or exceed int32 keys", views, height, width);
    SNERF_REQUIRE(min_views >= 1 && min_views <= views, "visibility_mask_combine: min_views %d outside 1..%d", min_views, views);
    const long long pixels = (long long)height * width;
    hipLaunchKernelGGL(combine_kernel, dim3(snerf::stride_grid(pixels, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, mask_views, views,
                       pixels, min_views, mask);
    return snerf::check_launch("visibility_mask_combine");
}
