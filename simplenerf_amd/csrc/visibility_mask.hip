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
#include "splat_project.h"

namespace {

using namespace snerf::splat;

constexpr int kBlock = kProjectBlock;

// (project: project_kernel of splat_project.h, shared with the Warper; here without a source mask and without the flow)

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
    hipLaunchKernelGGL(project_kernel, dim3(blocks, views), dim3(kBlock), 0, (hipStream_t)stream, depth_train, cameras,
                       (const unsigned char*)nullptr, height, width, points, keys, (double*)nullptr, partials);
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
