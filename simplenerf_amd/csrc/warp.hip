// Q5: the reference's Warper (src/qa/00_Common/src/mask_generators/Warper.py) beyond the depth-only splat of the visibility masks:
// forward_warp's colour frame and flow, bilinear_splatting of any (h, w, c) frame along any flow with a source mask and a flow mask,
// and bilinear_interpolation, the backward warp.
//
// The splat is the masks' (visibility_mask.hip): sources are keyed by their unclipped floor cell, the caller sorts the keys (stable)
// and finds the list starts with the masks' entry points, and one thread per destination pixel walks its four lists in a fixed order
// (splat_cells.h, warp_cells.h) -- no atomics, the same bits on every call.  A source that its mask or its flow mask drops takes the
// discard key: the reference multiplies its weight by 0, which adds nothing either.  max L is taken over ALL pixels of the depth,
// dropped ones included, as the reference's log_depth1.max() is.  The backward warp has no lists: one thread per pixel reads four taps.
// All arithmetic is fp64 on inputs widened first, compiled without FMA contraction (the build's -ffp-contract=off): a position
// computed from a flow, and every output of the backward warp, is numpy's bit for bit.  Bound: the gather by fp64 divide / exp / log
// rate, everything else by memory.
#include <cmath>

#include "snerf_common.h"
#include "splat_cells.h"
#include "splat_project.h"
#include "warp_cells.h"

namespace {

using namespace snerf::splat;

constexpr int kBlock = kProjectBlock;

__device__ __forceinline__ bool kept(const unsigned char* __restrict__ mask, long long i) { return !mask || mask[i] != 0; }

// ------------------------------------------------------------------------------------------------ positions
// One view.  points = planes X, Y, Z; keys = the source's list (the discard key where a mask drops it); partial = (max L, max Z) of
// the workgroup's pixels.
template <typename D>
__global__ void __launch_bounds__(kBlock) positions_from_flow_kernel(const double* __restrict__ flow, const D* __restrict__ depth,
                                                                     const unsigned char* __restrict__ mask1,
                                                                     const unsigned char* __restrict__ flow_mask, int height, int width,
                                                                     double* __restrict__ points, int* __restrict__ keys,
                                                                     double* __restrict__ partials) {
    __shared__ double lds[kProjectWaves];
    const long long n = (long long)height * width;
    double* px = points;
    double* py = px + n;
    double* pz = py + n;
    double max_l = 0.0, max_d = -INFINITY;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int yi = (int)(i / width), xi = (int)(i - (long long)yi * width);
        const double X = (flow[2 * i] + (double)xi) + 1.0, Y = (flow[2 * i + 1] + (double)yi) + 1.0, Z = (double)depth[i];
        px[i] = X;
        py[i] = Y;
        pz[i] = Z;
        keys[i] = (kept(mask1, i) && kept(flow_mask, i)) ? source_key(X, Y, Z, height, width) : cell_keys(height, width);
        max_l = fmax(max_l, log_depth(Z));
        max_d = fmax(max_d, Z);
    }
    max_l = block_max(max_l, lds);
    max_d = block_max(max_d, lds);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = max_l;
        partials[2 * blockIdx.x + 1] = max_d;
    }
}

// ------------------------------------------------------------------------------------------------ splat gather
// One thread per destination pixel: the padded cell (y + 1, x + 1) sums what the sources of its four lists add to it, list by list,
// each list in ascending source order, each source's corners in the order nw, sw, ne, se -- the masks' gather with `channels` values
// per source where that one has Z.
template <typename T>
__global__ void __launch_bounds__(kBlock) splat_gather_kernel(const double* __restrict__ points, const long long* __restrict__ order,
                                                              const int* __restrict__ starts, const double* __restrict__ stats,
                                                              const T* __restrict__ values, int channels, int is_image, int height,
                                                              int width, void* __restrict__ warped, unsigned char* __restrict__ mask2) {
    const long long n = (long long)height * width;
    const double max_l = stats[0];
    const double* px = points;
    const double* py = px + n;
    const double* pz = py + n;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int y = (int)(i / width), x = (int)(i - (long long)y * width);
        double sum[4] = {0.0, 0.0, 0.0, 0.0}, ws = 0.0;
        if (max_l > 0.0) {   // (max L = 0: every weight is 0 / 0 in the reference; nothing is added here)
            int lists[4];
            const int num_lists = lists_of(y + 1, x + 1, width, lists);
            for (int l = 0; l < num_lists; ++l) {
                const int first = starts[lists[l]], last = starts[lists[l] + 1];
                for (int s = first; s < last; ++s) {
                    const long long source = order[s];
                    if (source < 0 || source >= n) continue;   // (not an index of this frame: an `order` that is no sort of `keys`)
                    double k[4];
                    const int corners = corner_weights(px[source], py[source], depth_divisor(pz[source], max_l), y + 1, x + 1, height, width, k);
                    if (corners == 0) continue;
                    double v[4];
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) v[ch] = ch < channels ? (double)values[source * channels + ch] : 0.0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (j < corners) {
#pragma unroll
                            for (int ch = 0; ch < 4; ++ch) sum[ch] += v[ch] * k[j];
                            ws += k[j];
                        }
                    }
                }
            }
        }
        const bool landed = ws > 0.0;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (ch < channels) {
                const double value = landed ? sum[ch] / ws : 0.0;
                if (is_image) ((unsigned char*)warped)[i * channels + ch] = to_image(value);
                else ((double*)warped)[i * channels + ch] = value;
            }
        }
        mask2[i] = landed ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ backward warp
// One thread per pixel: four taps of the zero-padded frame2 / mask2 at the flowed position, nr and dr summed nw, sw, ne, se.  A
// position that is not finite or leaves int32 (undefined in the reference) reads nothing: value 0, mask 0.
template <typename T>
__global__ void __launch_bounds__(kBlock) interpolate_kernel(const T* __restrict__ frame2, const unsigned char* __restrict__ mask2,
                                                             const double* __restrict__ flow, const unsigned char* __restrict__ flow_mask,
                                                             int channels, int is_image, int height, int width, void* __restrict__ warped,
                                                             unsigned char* __restrict__ mask1) {
    const long long n = (long long)height * width;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int yi = (int)(i / width), xi = (int)(i - (long long)yi * width);
        const double X = (flow[2 * i] + (double)xi) + 1.0, Y = (flow[2 * i + 1] + (double)yi) + 1.0;
        double nr[4] = {0.0, 0.0, 0.0, 0.0}, dr = 0.0;
        if (pinned(X) && pinned(Y)) {
            const Taps taps = taps_of(X, Y, height, width);
            const double valid = kept(flow_mask, i) ? 1.0 : 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long tap = frame_index(taps.row[j], taps.col[j], height, width);
                const double weight = taps.prox[j] * valid;
                const double m = (tap >= 0 && kept(mask2, tap)) ? 1.0 : 0.0;
                // (the first term starts the sum, as in the reference's a + b + c + d: 0 + a would turn a -0 into +0)
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    if (ch < channels) {
                        const double term = weight * (tap >= 0 ? (double)frame2[tap * channels + ch] : 0.0) * m;
                        nr[ch] = j == 0 ? term : nr[ch] + term;
                    }
                }
                dr = j == 0 ? weight * m : dr + weight * m;
            }
        }
        const bool known = dr > 0.0;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (ch < channels) {
                const double value = known ? nr[ch] / dr : 0.0;
                if (is_image) ((unsigned char*)warped)[i * channels + ch] = to_image(value);
                else ((double*)warped)[i * channels + ch] = value;
            }
        }
        mask1[i] = known ? 1 : 0;
    }
}

inline bool frame_fits(int height, int width) { return fits(1, height, width); }

inline bool values_fit(int value_type, int channels, int is_image) {
    if (channels < 1 || channels > 4) return false;
    if (value_type != SNERF_WARP_U8 && value_type != SNERF_WARP_F32 && value_type != SNERF_WARP_F64) return false;
    return !is_image || value_type == SNERF_WARP_U8;
}

}  // namespace

extern "C" long long snerf_warp_workspace_bytes(int height, int width) {
    if (!frame_fits(height, width)) return 0;
    return (long long)kMaxPartials * 2 * 8;
}

extern "C" int snerf_warp_project(const float* depth1, const double* camera, const unsigned char* mask1, int height, int width,
                                  double* points, int* keys, double* stats, double* flow12, void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(depth1 && camera && points && keys && stats && flow12 && workspace, "warp_project: NULL pointer");
    SNERF_REQUIRE(frame_fits(height, width), "warp_project: a frame of %d x %d is empty or exceeds int32 keys", height, width);
    const int blocks = project_blocks((long long)height * width);
    double* partials = (double*)workspace;
    hipLaunchKernelGGL(project_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, depth1, camera, mask1, height, width, points, keys,
                       flow12, partials);
    hipLaunchKernelGGL(fold_max_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const double*)partials, blocks, stats);
    return snerf::check_launch("warp_project");
}

extern "C" int snerf_warp_positions_from_flow(const double* flow12, const void* depth1, int depth_type, const unsigned char* mask1,
                                              const unsigned char* flow12_mask, int height, int width, double* points, int* keys,
                                              double* stats, void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(flow12 && depth1 && points && keys && stats && workspace, "warp_positions_from_flow: NULL pointer");
    SNERF_REQUIRE(depth_type == SNERF_WARP_F32 || depth_type == SNERF_WARP_F64,
                  "warp_positions_from_flow: depth_type %d is neither SNERF_WARP_F32 nor SNERF_WARP_F64", depth_type);
    SNERF_REQUIRE(frame_fits(height, width), "warp_positions_from_flow: a frame of %d x %d is empty or exceeds int32 keys", height, width);
    const int blocks = project_blocks((long long)height * width);
    double* partials = (double*)workspace;
    if (depth_type == SNERF_WARP_F32)
        hipLaunchKernelGGL(positions_from_flow_kernel<float>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, flow12,
                           (const float*)depth1, mask1, flow12_mask, height, width, points, keys, partials);
    else
        hipLaunchKernelGGL(positions_from_flow_kernel<double>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, flow12,
                           (const double*)depth1, mask1, flow12_mask, height, width, points, keys, partials);
    hipLaunchKernelGGL(fold_max_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const double*)partials, blocks, stats);
    return snerf::check_launch("warp_positions_from_flow");
}

extern "C" int snerf_warp_splat_gather(const double* points, const long long* order, const int* starts, const double* stats,
                                       const void* values, int value_type, int channels, int is_image, int height, int width,
                                       void* warped, unsigned char* mask2, snerf_stream_t stream) {
    SNERF_REQUIRE(points && order && starts && stats && values && warped && mask2, "warp_splat_gather: NULL pointer");
    SNERF_REQUIRE(frame_fits(height, width), "warp_splat_gather: a frame of %d x %d is empty or exceeds int32 keys", height, width);
    SNERF_REQUIRE(values_fit(value_type, channels, is_image),
                  "warp_splat_gather: value_type %d with %d channels and is_image %d: expected 1..4 channels of SNERF_WARP_U8 / F32 / F64, "
                  "is_image only with SNERF_WARP_U8", value_type, channels, is_image);
    const dim3 grid(snerf::stride_grid((long long)height * width, kBlock)), block(kBlock);
    if (value_type == SNERF_WARP_U8)
        hipLaunchKernelGGL(splat_gather_kernel<unsigned char>, grid, block, 0, (hipStream_t)stream, points, order, starts, stats,
                           (const unsigned char*)values, channels, is_image, height, width, warped, mask2);
    else if (value_type == SNERF_WARP_F32)
        hipLaunchKernelGGL(splat_gather_kernel<float>, grid, block, 0, (hipStream_t)stream, points, order, starts, stats,
                           (const float*)values, channels, is_image, height, width, warped, mask2);
    else
        hipLaunchKernelGGL(splat_gather_kernel<double>, grid, block, 0, (hipStream_t)stream, points, order, starts, stats,
                           (const double*)values, channels, is_image, height, width, warped, mask2);
    return snerf::check_launch("warp_splat_gather");
}

extern "C" int snerf_warp_interpolate(const void* frame2, int value_type, int channels, const unsigned char* mask2, const double* flow12,
                                      const unsigned char* flow12_mask, int is_image, int height, int width, void* warped,
                                      unsigned char* mask1, snerf_stream_t stream) {
    SNERF_REQUIRE(frame2 && flow12 && warped && mask1, "warp_interpolate: NULL pointer");
    SNERF_REQUIRE(frame_fits(height, width), "warp_interpolate: a frame of %d x %d is empty or exceeds int32 keys", height, width);
    SNERF_REQUIRE(values_fit(value_type, channels, is_image),
                  "warp_interpolate: value_type %d with %d channels and is_image %d: expected 1..4 channels of SNERF_WARP_U8 / F32 / F64, "
                  "is_image only with SNERF_WARP_U8", value_type, channels, is_image);
    const dim3 grid(snerf::stride_grid((long long)height * width, kBlock)), block(kBlock);
    if (value_type == SNERF_WARP_U8)
        hipLaunchKernelGGL(interpolate_kernel<unsigned char>, grid, block, 0, (hipStream_t)stream, (const unsigned char*)frame2, mask2, flow12,
                           flow12_mask, channels, is_image, height, width, warped, mask1);
    else if (value_type == SNERF_WARP_F32)
        hipLaunchKernelGGL(interpolate_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)frame2, mask2, flow12, flow12_mask,
                           channels, is_image, height, width, warped, mask1);
    else
        hipLaunchKernelGGL(interpolate_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)frame2, mask2, flow12, flow12_mask,
                           channels, is_image, height, width, warped, mask1);
    return snerf::check_launch("warp_interpolate");
}
