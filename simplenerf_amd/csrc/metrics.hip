// Q1: scoring rendered frames on the device (the reference's third stage, src/qa/*: RMSE / PSNR / SSIM of the 8-bit frame,
// MAE / RMSE / SROCC of the depth map, plain and masked).  The inputs are what the renderer leaves on the device -- the uint8
// image of snerf_to_display and fp32 depths -- and only a handful of sums leave it; the host turns them into the metrics with the
// reference's own expressions (simplenerf_amd/qa.py).
//
// Arithmetic: image error sums are exact 64-bit integers; everything else is fp64 (the SSIM variance is E[x^2] - E[x]^2 with
// E[x^2] up to 65 025 against a floor of C2 = 58.5: fp32 is 2.7e-6 off on a bright smooth image).  Every reduction is thread ->
// wave (xor shuffles) -> workgroup (LDS, wave order) -> one partial per workgroup in the caller's workspace -> a second launch
// of ONE workgroup that folds the partials in a fixed order.  No atomics: two calls on one input return the same bits.
// This file holds no fp32 arithmetic (floats are widened on load), so the packed-fp32 operand-selection hazard of build.py's
// FILE_FLAGS cannot arise here.  Bound: the SSIM kernel by LDS reads / fp64 FMAs, the rest by launch latency.
#include <cmath>
#include <type_traits>

#include "block_reduce.h"
#include "metrics_tile.h"
#include "snerf_common.h"

namespace {

using namespace snerf::ssim_tile;

using namespace snerf::reduce;          // kBlock, kWaves, wave_sum_t, block_sum (shared with csrc/lpips.hip)

constexpr int kMaxPartials = 1024;   // workgroups of a 1-D reduction
constexpr int kMaxSums = 4;          // values per workgroup of a 1-D reduction

// Second launch of every reduction: ONE workgroup; out[j] = sum over b of partials[b * width + j], thread t taking b = t,
// t + kBlock, ... in order, then block_sum.  `sorted` (depth sums only): also out[width] = numpy.median of sorted * scale.
template <typename T>
__global__ void __launch_bounds__(kBlock) fold_kernel(const T* __restrict__ partials, int num_partials, int width,
                                                      T* __restrict__ out, const float* __restrict__ sorted, long long count,
                                                      double scale) {
    __shared__ T lds[kWaves];
    for (int j = 0; j < width; ++j) {
        T s = 0;
        for (int b = threadIdx.x; b < num_partials; b += kBlock) s += partials[(long long)b * width + j];
        s = block_sum(s, lds);
        if (threadIdx.x == 0) out[j] = s;
    }
    if constexpr (std::is_same<T, double>::value) {
        if (sorted && threadIdx.x == 0 && count > 0) {
            // numpy.median: the middle value, or numpy.mean of the two middle values (their sum, divided by 2)
            const double hi = (double)sorted[count / 2] * scale;
            out[width] = (count & 1) ? hi : ((double)sorted[count / 2 - 1] * scale + hi) / 2.0;
        }
    }
}

inline int reduction_blocks(long long count) {
    long long blocks = (count + kBlock - 1) / kBlock;
    if (blocks > kMaxPartials) blocks = kMaxPartials;
    return blocks < 1 ? 1 : (int)blocks;
}

// ------------------------------------------------------------------------------------------------ image error sums
// partial = (sum (gt - eval)^2 over all 3 channels, the same over masked pixels, number of masked pixels)
__global__ void __launch_bounds__(kBlock) image_error_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ eval,
                                                             const unsigned char* __restrict__ mask, long long pixels,
                                                             long long* __restrict__ partials) {
    __shared__ long long lds[kWaves];
    long long all = 0, masked = 0, kept = 0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < pixels; i += stride) {
        int sq = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int d = (int)gt[3 * i + c] - (int)eval[3 * i + c];
            sq += d * d;
        }
        all += sq;
        if (mask && mask[i]) {
            masked += sq;
            kept += 1;
        }
    }
    all = block_sum(all, lds);
    masked = block_sum(masked, lds);
    kept = block_sum(kept, lds);
    if (threadIdx.x == 0) {
        partials[3 * blockIdx.x + 0] = all;
        partials[3 * blockIdx.x + 1] = masked;
        partials[3 * blockIdx.x + 2] = kept;
    }
}

// ------------------------------------------------------------------------------------------------ SSIM
// One workgroup owns a kTileH x kTileW output tile.  Both images' tile plus a kRadius halo (all three channels, bytes) go to LDS
// with scipy's `reflect` boundary applied while loading (metrics_tile.h); per channel the five moment inputs (x, y, x^2, y^2,
// xy) are filtered along the rows into fp64 LDS maps of (kTileH + 2 kRadius) x kTileW, then along the columns into registers.
// A row of a map is 32 doubles = one 256-byte bank row: the 32 lanes of a half-wave read it conflict-free with ds_read_b64.
// 40 KB of LDS and 64 VGPRs: four workgroups per CU.
static_assert(kTileW * kTileH == 2 * kBlock, "two output pixels per thread");

struct SsimParams {
    double w[kTaps];   // scipy.ndimage's normalised Gaussian, sigma = 1.5
    double c1, c2;     // (0.01 * 255)^2, (0.03 * 255)^2
};

__global__ void __launch_bounds__(kBlock) ssim_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ eval,
                                                      const unsigned char* __restrict__ mask, int height, int width, SsimParams p,
                                                      double* __restrict__ s_map, double* __restrict__ partials) {
    __shared__ unsigned char in_x[kInH][kInPitch];
    __shared__ unsigned char in_y[kInH][kInPitch];
    __shared__ double rows[5][kInH][kTileW];
    __shared__ double lds[kWaves];
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;

    for (int i = threadIdx.x; i < kInH * kInW * 3; i += kBlock) {
        const int r = i / (kInW * 3), b = i - r * (kInW * 3), col = b / 3, c = b - 3 * col;
        const int sy = source_index(y0, r, height), sx = source_index(x0, col, width);
        const long long pixel = (long long)sy * width + sx;
        const unsigned char x = gt[3 * pixel + c];
        in_x[r][b] = x;
        in_y[r][b] = (mask && !mask[pixel]) ? x : eval[3 * pixel + c];   // MaskedSSIM: eval' = m ? eval : gt
    }

    const int tx = threadIdx.x & (kTileW - 1), ty = threadIdx.x / kTileW;   // pixels (ty, tx) and (ty + kTileH / 2, tx)
    double cropped = 0.0, weighted = 0.0;
    for (int c = 0; c < 3; ++c) {
        __syncthreads();   // inputs loaded / the previous channel's maps have been read
        for (int i = threadIdx.x; i < kInH * kTileW; i += kBlock) {
            const int r = i / kTileW, col = i - r * kTileW;
            double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const double x = (double)in_x[r][3 * (col + k) + c], y = (double)in_y[r][3 * (col + k) + c];
                m[0] += p.w[k] * x;
                m[1] += p.w[k] * y;
                m[2] += p.w[k] * (x * x);
                m[3] += p.w[k] * (y * y);
                m[4] += p.w[k] * (x * y);
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) rows[j][r][col] = m[j];
        }
        __syncthreads();
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int oy = ty + half * (kTileH / 2);
            double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
#pragma unroll
                for (int j = 0; j < 5; ++j) m[j] += p.w[k] * rows[j][oy + k][tx];
            }
            const int gy = y0 + oy, gx = x0 + tx;
            if (gy < height && gx < width) {
                const double ux = m[0], uy = m[1];
                const double vx = m[2] - ux * ux, vy = m[3] - uy * uy, vxy = m[4] - ux * uy;
                const double a1 = 2.0 * ux * uy + p.c1, a2 = 2.0 * vxy + p.c2;
                const double b1 = ux * ux + uy * uy + p.c1, b2 = vx + vy + p.c2;
                const double s = (a1 * a2) / (b1 * b2);
                const long long pixel = (long long)gy * width + gx;
                if (s_map) s_map[3 * pixel + c] = s;
                if (gy >= kRadius && gy < height - kRadius && gx >= kRadius && gx < width - kRadius) cropped += s;
                if (!mask || mask[pixel]) weighted += s;
            }
        }
    }
    cropped = block_sum(cropped, lds);
    weighted = block_sum(weighted, lds);
    if (threadIdx.x == 0) {
        const long long tile = (long long)blockIdx.y * gridDim.x + blockIdx.x;
        partials[2 * tile + 0] = cropped;
        partials[2 * tile + 1] = weighted;
    }
}

// ------------------------------------------------------------------------------------------------ depth error sums
// e = gt * gt_scale - eval * eval_scale in fp64 on (mask or every) pixel: partial = (sum |e|, sum e^2, pixels counted)
__global__ void __launch_bounds__(kBlock) depth_error_kernel(const float* __restrict__ gt, const float* __restrict__ eval, double gt_scale,
                                                             double eval_scale, const unsigned char* __restrict__ mask, long long count,
                                                             double* __restrict__ partials) {
    __shared__ double lds[kWaves];
    double abs_sum = 0.0, sq_sum = 0.0, kept = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        if (mask && !mask[i]) continue;
        const double e = (double)gt[i] * gt_scale - (double)eval[i] * eval_scale;
        abs_sum += fabs(e);
        sq_sum += e * e;
        kept += 1.0;
    }
    abs_sum = block_sum(abs_sum, lds);
    sq_sum = block_sum(sq_sum, lds);
    kept = block_sum(kept, lds);
    if (threadIdx.x == 0) {
        partials[3 * blockIdx.x + 0] = abs_sum;
        partials[3 * blockIdx.x + 1] = sq_sum;
        partials[3 * blockIdx.x + 2] = kept;
    }
}

// ------------------------------------------------------------------------------------------------ rank correlation sums
// Tie-averaged rank of v among `sorted` (ascending, `count` values), minus the mean rank (count + 1) / 2: the values equal to v
// occupy the 1-based ranks lower + 1 .. upper, whose mean is (lower + upper + 1) / 2.  Two binary searches: a run of 10^5 equal
// depths costs what any other value costs.
__device__ __forceinline__ double centred_rank(const float* __restrict__ sorted, long long count, float v) {
    long long lo = 0, hi = count;
    while (lo < hi) {   // lower bound: first index with sorted[i] >= v
        const long long mid = lo + (hi - lo) / 2;
        if (sorted[mid] < v) lo = mid + 1; else hi = mid;
    }
    const long long lower = lo;
    hi = count;
    while (lo < hi) {   // upper bound: first index with sorted[i] > v
        const long long mid = lo + (hi - lo) / 2;
        if (sorted[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return 0.5 * (double)(lower + lo - count);   // (lower + upper + 1) / 2 - (count + 1) / 2: a multiple of 0.5, exact
}

// partial = (sum rx ry, sum rx^2, sum ry^2) of the centred ranks
__global__ void __launch_bounds__(kBlock) rank_correlation_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                  const float* __restrict__ sorted_x, const float* __restrict__ sorted_y,
                                                                  long long count, double* __restrict__ partials) {
    __shared__ double lds[kWaves];
    double sxy = 0.0, sxx = 0.0, syy = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        const double rx = centred_rank(sorted_x, count, x[i]), ry = centred_rank(sorted_y, count, y[i]);
        sxy += rx * ry;
        sxx += rx * rx;
        syy += ry * ry;
    }
    sxy = block_sum(sxy, lds);
    sxx = block_sum(sxx, lds);
    syy = block_sum(syy, lds);
    if (threadIdx.x == 0) {
        partials[3 * blockIdx.x + 0] = sxy;
        partials[3 * blockIdx.x + 1] = sxx;
        partials[3 * blockIdx.x + 2] = syy;
    }
}

inline long long ssim_tiles_x(int width) { return (width + kTileW - 1) / kTileW; }
inline long long ssim_tiles_y(int height) { return (height + kTileH - 1) / kTileH; }

}  // namespace

extern "C" long long snerf_metrics_workspace_bytes(int height, int width) {
    if (height < 1 || width < 1) return 0;
    const long long tiles = ssim_tiles_x(width) * ssim_tiles_y(height) * 2;
    const long long flat = (long long)kMaxPartials * kMaxSums;
    return 8 * (tiles > flat ? tiles : flat);
}

extern "C" int snerf_image_error_sums(const unsigned char* gt, const unsigned char* eval, const unsigned char* mask, int height,
                                      int width, long long* sums, void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(gt && eval && sums && workspace, "image_error_sums: NULL pointer");
    SNERF_REQUIRE(height >= 1 && width >= 1, "image_error_sums: empty image (%d x %d)", height, width);
    const long long pixels = (long long)height * width;
    const int blocks = reduction_blocks(pixels);
    long long* partials = (long long*)workspace;
    hipLaunchKernelGGL(image_error_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, gt, eval, mask, pixels, partials);
    hipLaunchKernelGGL(fold_kernel<long long>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const long long*)partials, blocks, 3,
                       sums, (const float*)nullptr, 0LL, 0.0);
    return snerf::check_launch("image_error_sums");
}

extern "C" int snerf_ssim_sums(const unsigned char* gt, const unsigned char* eval, const unsigned char* mask, int height, int width,
                               double* sums, double* s_map, void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(gt && eval && sums && workspace, "ssim_sums: NULL pointer");
    // skimage: "win_size exceeds image extent" -- the 11-tap window must fit, and one reflection must reach every tap
    SNERF_REQUIRE(height >= kTaps && width >= kTaps, "ssim_sums: a %d x %d image is smaller than the %d-tap window", height, width, kTaps);
    const long long tiles_x = ssim_tiles_x(width), tiles_y = ssim_tiles_y(height);
    SNERF_REQUIRE(tiles_y <= 65535, "ssim_sums: height %d exceeds the grid", height);
    SsimParams p;
    double total = 0.0;
    for (int k = 0; k < kTaps; ++k) {   // scipy.ndimage._gaussian_kernel1d: exp(-0.5 / sigma^2 * x^2), normalised by its sum
        const double x = (double)(k - kRadius);
        p.w[k] = exp(-0.5 / (1.5 * 1.5) * (x * x));
        total += p.w[k];
    }
    for (int k = 0; k < kTaps; ++k) p.w[k] /= total;
    p.c1 = (0.01 * 255.0) * (0.01 * 255.0);
    p.c2 = (0.03 * 255.0) * (0.03 * 255.0);
    double* partials = (double*)workspace;
    hipLaunchKernelGGL(ssim_kernel, dim3((unsigned)tiles_x, (unsigned)tiles_y), dim3(kBlock), 0, (hipStream_t)stream, gt, eval, mask,
                       height, width, p, s_map, partials);
    hipLaunchKernelGGL(fold_kernel<double>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const double*)partials,
                       (int)(tiles_x * tiles_y), 2, sums, (const float*)nullptr, 0LL, 0.0);
    return snerf::check_launch("ssim_sums");
}

extern "C" int snerf_depth_error_sums(const float* gt, const float* eval, double gt_scale, double eval_scale,
                                      const unsigned char* mask, long long count, const float* sorted_gt, double* sums,
                                      void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(gt && eval && sums && workspace, "depth_error_sums: NULL pointer");
    SNERF_REQUIRE(count >= 1, "depth_error_sums: empty depth map");
    const int blocks = reduction_blocks(count);
    double* partials = (double*)workspace;
    hipLaunchKernelGGL(depth_error_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, gt, eval, gt_scale, eval_scale, mask,
                       count, partials);
    hipLaunchKernelGGL(fold_kernel<double>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const double*)partials, blocks, 3, sums,
                       sorted_gt, count, gt_scale);
    return snerf::check_launch("depth_error_sums");
}

extern "C" int snerf_rank_correlation_sums(const float* x, const float* y, const float* sorted_x, const float* sorted_y,
                                           long long count, double* sums, void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(x && y && sorted_x && sorted_y && sums && workspace, "rank_correlation_sums: NULL pointer");
    SNERF_REQUIRE(count >= 1, "rank_correlation_sums: no values");
    const int blocks = reduction_blocks(count);
    double* partials = (double*)workspace;
    hipLaunchKernelGGL(rank_correlation_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, x, y, sorted_x, sorted_y, count,
                       partials);
    hipLaunchKernelGGL(fold_kernel<double>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const double*)partials, blocks, 3, sums,
                       (const float*)nullptr, 0LL, 0.0);
    return snerf::check_launch("rank_correlation_sums");
}
