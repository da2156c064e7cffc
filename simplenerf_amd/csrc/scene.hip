// S1-S3: the scene tables on the device, from what the data loader returns.  Restates the per-pixel parts of the
// reference's DataPreprocessor (src/data_preprocessors/DataPreprocessor01.py): preprocess_images :929-935, the COLMAP-point
// rasterisation of preprocess_raw_sparse_depth_data :163-185 and convert_depth_to_ndc :455-463 as preprocess_sparse_depth_data
// :448-452 and preprocess_dense_depth_data :474-478 call it.  Start-up streaming work: every output is a pure function of the
// inputs (integer atomics only), in the reference's fp32 / fp64 operation order, so the tables are bit-identical to numpy's.
#include "snerf_common.h"
#include "raygen_device.h"

#include "../../include/simplenerf_train.h"

namespace {

// (V,h,w,C) uint8 -> (V,h,w,3) fp32: images.astype('float32') / 255, then [..., :3] * a + (1. - a) with a = the LAST channel
// (:932; the alpha of an RGBA image) when white_bkgd, else [..., :3].
__global__ void __launch_bounds__(256) scene_images_kernel(const unsigned char* __restrict__ images, long long num_pixels, int channels,
                                                           int white_bkgd, float* __restrict__ out) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < num_pixels; i += stride) {
        const unsigned char* px = images + i * channels;
        float rgb[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = __fdiv_rn((float)px[c], 255.0f);
        if (white_bkgd) {
            const float a = __fdiv_rn((float)px[channels - 1], 255.0f);
            const float rest = 1.0f - a;
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c] = rgb[c] * a + rest;
        }
        out[3 * i] = rgb[0]; out[3 * i + 1] = rgb[1]; out[3 * i + 2] = rgb[2];
    }
}

// Pass 1 of the rasteriser: the pixel of every point (numpy.clip(numpy.round(x / divisor), 0, w-1).astype('int'), :175-178) and
// the LARGEST point index per pixel -- numpy's fancy assignment keeps the last of several points on one pixel (:179-180).
__global__ void __launch_bounds__(256) sparse_winner_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                            const int* __restrict__ view, long long num_points, double divisor,
                                                            int num_views, int height, int width, int* __restrict__ winner) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < num_points; p += stride) {
        const int v = view[p];
        const double rx = rint(x[p] / divisor), ry = rint(y[p] / divisor);      // round half to even, like numpy.round
        if (v < 0 || v >= num_views || rx != rx || ry != ry) continue;           // no pixel: dropped (the header says why)
        const int px = (int)fmin(fmax(rx, 0.0), (double)(width - 1));            // clipped BEFORE the integer conversion
        const int py = (int)fmin(fmax(ry, 0.0), (double)(height - 1));
        atomicMax(winner + ((long long)v * height + py) * width + px, (int)p);
    }
}

// convert_depth_to_ndc (:456-463) for one pixel, fp32 in the reference's order; oz, dz = the z of the pixel's world ray.
__device__ __forceinline__ float depth_to_ndc(const snerf::Camera& cam, int px, int py, float near, float depth) {
    float o[3], d[3];
    snerf::pinhole_ray(cam, (float)px, (float)py, near, false, o, d, nullptr, nullptr, nullptr);
    const float oz = o[2], dz = d[2];
    const float tn = __fdiv_rn(-(near + oz), dz);
    const float oz_prime = oz + tn * dz;
    const float ndc = 1.0f - __fdiv_rn(oz_prime, oz_prime + (depth - tn) * dz);
    return depth == -1.0f ? -1.0f : ndc;       // depths_ndc[depths == -1] = -1 (:451, :477)
}

// Pass 2: one thread per pixel writes the winner's values (depth * sc in fp64, then float32: :179, :439-440) or -1, and the NDC
// depth of the same fp32 value when a camera table is given.
__global__ void __launch_bounds__(256) sparse_tables_kernel(const int* __restrict__ winner, const double* __restrict__ depth,
                                                            const double* __restrict__ error, long long num_points, double scale,
                                                            const snerf::Camera* __restrict__ cameras, float near, long long num_pixels,
                                                            int height, int width, float* __restrict__ depths,
                                                            float* __restrict__ errors, float* __restrict__ depths_ndc) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long frame = (long long)height * width;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < num_pixels; i += stride) {
        const long long p = winner[i];
        const bool hit = p >= 0 && p < num_points;
        const float value = hit ? (float)(depth[p] * scale) : -1.0f;
        depths[i] = value;
        errors[i] = hit ? (float)error[p] : -1.0f;
        if (depths_ndc) {
            const long long v = i / frame;
            const int pix = (int)(i - v * frame);
            const int py = pix / width, px = pix - py * width;
            depths_ndc[i] = depth_to_ndc(cameras[v], px, py, near, value);
        }
    }
}

__global__ void __launch_bounds__(256) depth_table_to_ndc_kernel(const float* __restrict__ depths, const snerf::Camera* __restrict__ cameras,
                                                                 float near, long long num_pixels, int height, int width,
                                                                 float* __restrict__ depths_ndc) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long frame = (long long)height * width;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < num_pixels; i += stride) {
        const long long v = i / frame;
        const int pix = (int)(i - v * frame);
        const int py = pix / width, px = pix - py * width;
        depths_ndc[i] = depth_to_ndc(cameras[v], px, py, near, depths[i]);
    }
}

int check_frame(const char* what, int num_views, int height, int width) {
    SNERF_REQUIRE(num_views >= 1 && height > 0 && width > 0, "%s: bad sizes (%d views, %dx%d)", what, num_views, height, width);
    return SNERF_OK;
}

}  // namespace

extern "C" int snerf_scene_images(const unsigned char* images, long long num_pixels, int channels, int white_bkgd, float* out,
                                  snerf_stream_t stream) {
    SNERF_REQUIRE(images && out, "scene_images: NULL pointer");
    SNERF_REQUIRE(channels == 3 || channels == 4, "scene_images: %d channels (3 or 4)", channels);
    SNERF_REQUIRE(num_pixels >= 0, "scene_images: %lld pixels", num_pixels);
    if (num_pixels == 0) return SNERF_OK;
    hipLaunchKernelGGL(scene_images_kernel, dim3(snerf::stride_grid(num_pixels, 256)), dim3(256), 0, (hipStream_t)stream, images,
                       num_pixels, channels, white_bkgd ? 1 : 0, out);
    return snerf::check_launch("scene_images");
}

extern "C" long long snerf_rasterise_sparse_depth_workspace_bytes(int num_views, int height, int width) {
    if (num_views < 1 || height < 1 || width < 1) return 0;
    return (long long)num_views * height * width * (long long)sizeof(int);
}

extern "C" int snerf_rasterise_sparse_depth(const double* x, const double* y, const double* depth, const double* reprojection_error,
                                            const int* view, long long num_points, double scale, double divisor,
                                            const float* camera_table, float near, int num_views, int height, int width,
                                            float* depths, float* errors, float* depths_ndc, void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(num_points >= 0 && num_points <= 0x7fffffffLL, "rasterise_sparse_depth: %lld points (at most 2^31-1: the winner "
                  "table holds int32 point indices)", num_points);
    SNERF_REQUIRE(num_points == 0 || (x && y && depth && reprojection_error && view), "rasterise_sparse_depth: NULL point array");
    SNERF_REQUIRE(depths && errors && workspace, "rasterise_sparse_depth: NULL output or workspace");
    SNERF_REQUIRE(!depths_ndc || camera_table, "rasterise_sparse_depth: an NDC table is wanted but the camera table is NULL");
    SNERF_REQUIRE(divisor > 0.0 && divisor <= 1.7976931348623157e308, "rasterise_sparse_depth: divisor %g is not a positive number",
                  divisor);
    if (int st = check_frame("rasterise_sparse_depth", num_views, height, width)) return st;
    const long long num_pixels = (long long)num_views * height * width;
    int* winner = static_cast<int*>(workspace);
    hipError_t e = hipMemsetAsync(winner, 0xff, (size_t)num_pixels * sizeof(int), (hipStream_t)stream);     // every pixel: -1
    if (e != hipSuccess) return snerf::fail(SNERF_E_HIP, "rasterise_sparse_depth: hipMemsetAsync: %s", hipGetErrorString(e));
    if (num_points > 0) {
        hipLaunchKernelGGL(sparse_winner_kernel, dim3(snerf::stride_grid(num_points, 256)), dim3(256), 0, (hipStream_t)stream, x, y,
                           view, num_points, divisor, num_views, height, width, winner);
        if (int st = snerf::check_launch("rasterise_sparse_depth (winners)")) return st;
    }
    hipLaunchKernelGGL(sparse_tables_kernel, dim3(snerf::stride_grid(num_pixels, 256)), dim3(256), 0, (hipStream_t)stream, winner, depth,
                       reprojection_error, num_points, scale, reinterpret_cast<const snerf::Camera*>(camera_table), near, num_pixels,
                       height, width, depths, errors, depths_ndc);
    return snerf::check_launch("rasterise_sparse_depth");
}

extern "C" int snerf_depth_table_to_ndc(const float* depths, const float* camera_table, int num_views, int height, int width,
                                        float near, float* depths_ndc, snerf_stream_t stream) {
    SNERF_REQUIRE(depths && camera_table && depths_ndc, "depth_table_to_ndc: NULL pointer");
    if (int st = check_frame("depth_table_to_ndc", num_views, height, width)) return st;
    const long long num_pixels = (long long)num_views * height * width;
    hipLaunchKernelGGL(depth_table_to_ndc_kernel, dim3(snerf::stride_grid(num_pixels, 256)), dim3(256), 0, (hipStream_t)stream, depths,
                       reinterpret_cast<const snerf::Camera*>(camera_table), near, num_pixels, height, width, depths_ndc);
    return snerf::check_launch("depth_table_to_ndc");
}
