// Normal maps (simplenerf_normals.h): the samples of a render that carry weight, the field's normals composited over them, the
// normals of a depth map, and normals as an 8-bit picture.
//
// snerf_ray_samples_count, two launches: a wave per ray (and one more for the total's slot) reads the ray's weights 64 at a time --
//   lane IS the sample order -- and adds the ballots' population counts; one workgroup scans the num_rays + 1 counts in place
//   (tile_scan.h's scan, the one fuse.hip and mesh.hip use).
// snerf_ray_samples_emit, one launch: the same wave walks the same ballots; a selected sample's position is the ray's offset + the
//   selected samples of the rounds before + those of the lower lanes, and its thread writes the flat index and the float32 point.
// snerf_composite_normals, one launch: a thread per ray walks its selected samples in order (sequential fp64 sums).
// snerf_depth_normals, one launch: a thread per pixel forms up to five points (fuse.hip's own unproject, fuse_point.h).
// snerf_normals_to_u8, one launch: a thread per normal.
// The inverse of the input map is here; the map's Jacobian is field.hip's own device function (field_map.h).  No atomics, one owner
// per output element, fp64 (the library is built with -ffp-contract=off) but the sample's point, which is the render's float32.
// Bound: the selection by memory (it reads every weight once per pass, 4 bytes a sample, coalesced); the compositing by memory
// latency -- a thread's samples are consecutive rows, a wave's are not -- and, with ndc, the fp64 divide rate (six divisions a
// sample); the depth normals by the fp64 multiply-add rate of five unprojections a pixel; the conversion by memory (15 bytes a
// normal).
#include <cmath>

#include "snerf_common.h"
#include "simplenerf_normals.h"
#include "field_map.h"
#include "fuse_point.h"
#include "sort_plan.h"
#include "tile_scan.h"

namespace {

using namespace snerf::sortplan;
using namespace snerf::tilescan;
using namespace snerf::fieldmap;
using namespace snerf::fusepoint;

__device__ __forceinline__ bool selected(float w, double min_weight) { return (double)w > min_weight; }     // (false for a NaN)

// ------------------------------------------------------------------------------------------------ the selection
// grid (ceil((num_rays + 1) / kWaves)): counts[ray] = the ray's selected samples, counts[num_rays] = 0
__global__ void __launch_bounds__(kBlock) ray_samples_count_kernel(const float* __restrict__ weights, long long num_rays, int num_samples,
                                                                   double min_weight, uint32_t* __restrict__ counts) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long long ray = (long long)blockIdx.x * kWaves + wave;      // (uniform over the wave)
    if (ray > num_rays) return;
    uint32_t held = 0;
    if (ray < num_rays) {
        const float* row = weights + ray * num_samples;
        for (int first = 0; first < num_samples; first += kWave) {
            const int i = first + lane;
            held += (uint32_t)__popcll(__ballot(i < num_samples && selected(row[i], min_weight)));
        }
    }
    if (lane == 0) counts[ray] = held;
}

// grid (ceil(num_rays / kWaves)): offsets scanned.  Selected sample (ray, i) goes to offsets[ray] + its position among the ray's.
__global__ void __launch_bounds__(kBlock) ray_samples_emit_kernel(const float* __restrict__ origins, const float* __restrict__ dirs,
                                                                  const float* __restrict__ z_vals, const float* __restrict__ weights,
                                                                  long long num_rays, int num_samples, double min_weight,
                                                                  const int* __restrict__ offsets, long long capacity,
                                                                  int* __restrict__ sample, float* __restrict__ points) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long long ray = (long long)blockIdx.x * kWaves + wave;      // (uniform over the wave)
    if (ray >= num_rays) return;
    const unsigned long long lower = (1ull << lane) - 1ull;
    const long long row = ray * num_samples;
    long long base = offsets[ray];
    float o[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = origins[3 * ray + a];
        d[a] = dirs[3 * ray + a];
    }
    for (int first = 0; first < num_samples; first += kWave) {
        const int i = first + lane;
        const bool mine = i < num_samples && selected(weights[row + i], min_weight);
        const unsigned long long round_selected = __ballot(mine);
        const long long to = base + (long long)__popcll(round_selected & lower);
        base += (long long)__popcll(round_selected);
        if (!mine || to < 0 || to >= capacity) continue;   // (outside: cannot happen with offsets of these weights; never write outside the buffers)
        const float z = z_vals[row + i];
        sample[to] = (int)(row + i);
#pragma unroll
        for (int a = 0; a < 3; ++a) points[3 * to + a] = o[a] + d[a] * z;      // float32: mul, rounded, then add (mlp_forward_body.h)
    }
}

// ------------------------------------------------------------------------------------------------ the compositing
// grid (ceil(num_rays / kBlock))
__global__ void __launch_bounds__(kBlock) composite_normals_kernel(const float* __restrict__ points, const float* __restrict__ grad,
                                                                   long long count, const int* __restrict__ offsets,
                                                                   const int* __restrict__ sample, const float* __restrict__ weights,
                                                                   long long num_rays, long long total, InputMap m,
                                                                   float* __restrict__ normal, float* __restrict__ strength) {
    const long long ray = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (ray >= num_rays) return;
    double A[3] = {0.0, 0.0, 0.0};
    const long long last = offsets[ray + 1];
    for (long long k = offsets[ray]; k < last; ++k) {
        if (k < 0 || k >= count) continue;                 // (offsets that are not this call's: never read outside the buffers)
        const long long at = sample[k];
        if (at < 0 || at >= total) continue;
        const double Q[3] = {(double)points[3 * k], (double)points[3 * k + 1], (double)points[3 * k + 2]};
        const double g[3] = {(double)grad[3 * k], (double)grad[3 * k + 1], (double)grad[3 * k + 2]};
        double P[3] = {Q[0], Q[1], Q[2]};
        bool usable = true;
        if (m.ndc) {                                       // the input map inverted
            P[2] = (2.0 * m.near) / (Q[2] - 1.0);
            P[0] = (Q[0] * P[2]) / m.cx;
            P[1] = (Q[1] * P[2]) / m.cy;
            usable = Q[2] < 1.0;                            // (a NaN fails; P_z <= -near is pull_back's own answer)
        }
        double G[3], length;
        usable = pull_back(m, P, g, G) && usable;
        usable = usable_length(G, &length) && usable;
        if (!usable) continue;
        const double w = (double)weights[at];
#pragma unroll
        for (int a = 0; a < 3; ++a) A[a] = A[a] + w * (-G[a] / length);
    }
    double s;
    const bool whole = usable_length(A, &s);
#pragma unroll
    for (int a = 0; a < 3; ++a) normal[3 * ray + a] = whole ? (float)(A[a] / s) : 0.0f;
    strength[ray] = whole ? (float)s : 0.0f;
}

// ------------------------------------------------------------------------------------------------ depth-map normals
struct DepthFrames {
    const float* depth;
    const unsigned char* mask;      // or NULL
    const double* cameras;
    int views, height, width;
    long long pixels, total;        // height * width, views * pixels
};

__device__ __forceinline__ bool valid_pixel(const DepthFrames& f, long long i) {
    return valid_depth(f.depth[i]) && (!f.mask || f.mask[i] != 0);
}

// Whether pixel (x, y) of the view whose first pixel is `first` is a usable neighbour of a valid pixel of depth d; its point if so.
__device__ __forceinline__ bool neighbour(const DepthFrames& f, const double* __restrict__ cam, long long first, int x, int y, double d,
                                          double edge_threshold, double P[3]) {
    if (x < 0 || x >= f.width || y < 0 || y >= f.height) return false;
    const long long j = first + (long long)y * f.width + x;
    if (!valid_pixel(f, j)) return false;
    const double other = (double)f.depth[j];
    if (edge_threshold >= 0.0 && !(fabs(other - d) <= edge_threshold * d)) return false;
    unproject(cam, x, y, other, P);
    return true;
}

// The tangent from the points before (a) and after (b) the pixel's own P along an axis: false when neither is usable.
__device__ __forceinline__ bool tangent(bool has_a, const double a[3], bool has_b, const double b[3], const double P[3], double t[3]) {
    if (!has_a && !has_b) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = has_a && has_b ? b[k] - a[k] : has_b ? b[k] - P[k] : P[k] - a[k];
    return true;
}

// grid (ceil(total / kBlock))
__global__ void __launch_bounds__(kBlock) depth_normals_kernel(DepthFrames f, double edge_threshold, float* __restrict__ normals) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= f.total) return;
    double n[3] = {0.0, 0.0, 0.0};
    if (valid_pixel(f, i)) {
        const int v = (int)(i / f.pixels);
        const long long first = (long long)v * f.pixels, pixel = i - first;
        const int y = (int)(pixel / f.width), x = (int)(pixel - (long long)y * f.width);
        const double* cam = f.cameras + (long long)v * kCamera;
        const double d = (double)f.depth[i];
        double P[3], left[3], right[3], above[3], below[3], tx[3], ty[3];
        unproject(cam, x, y, d, P);
        const bool has_left = neighbour(f, cam, first, x - 1, y, d, edge_threshold, left);
        const bool has_right = neighbour(f, cam, first, x + 1, y, d, edge_threshold, right);
        const bool has_above = neighbour(f, cam, first, x, y - 1, d, edge_threshold, above);
        const bool has_below = neighbour(f, cam, first, x, y + 1, d, edge_threshold, below);
        if (tangent(has_left, left, has_right, right, P, tx) && tangent(has_above, above, has_below, below, P, ty)) {
            const double c[3] = {tx[1] * ty[2] - tx[2] * ty[1], tx[2] * ty[0] - tx[0] * ty[2], tx[0] * ty[1] - tx[1] * ty[0]};
            double m;
            if (usable_length(c, &m)) {
#pragma unroll
                for (int a = 0; a < 3; ++a) n[a] = c[a] / m;
                const double* Ei = cam + kInvE;
                const double facing = (n[0] * (Ei[3] - P[0]) + n[1] * (Ei[7] - P[1])) + n[2] * (Ei[11] - P[2]);
                if (facing < 0.0) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) n[a] = -n[a];
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) normals[3 * i + a] = (float)n[a];
}

// ------------------------------------------------------------------------------------------------ the picture
struct Rotation {
    double r[9];
};

// grid (ceil(count / kBlock))
__global__ void __launch_bounds__(kBlock) normals_to_u8_kernel(const float* __restrict__ normals, long long count, Rotation R,
                                                               unsigned char* __restrict__ image) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const double n[3] = {(double)normals[3 * i], (double)normals[3 * i + 1], (double)normals[3 * i + 2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c = (R.r[a] * n[0] + R.r[3 + a] * n[1]) + R.r[6 + a] * n[2];
        const double level = floor(127.5 * (c + 1.0) + 0.5);
        image[3 * i + a] = (unsigned char)(level >= 255.0 ? 255 : level >= 0.0 ? (int)level : 0);     // (a NaN: 0)
    }
}

inline unsigned blocks_of(long long count, int per_block) { return (unsigned)((count + per_block - 1) / per_block); }

// SNERF_OK with *total = num_rays * num_samples, or the status the call returns (message set)
int samples_extent(const char* what, long long num_rays, int num_samples, long long* total) {
    SNERF_REQUIRE(num_rays >= 0 && num_samples >= 0, "%s: %lld rays of %d samples", what, num_rays, num_samples);
    if (num_rays > kMaxCount || (num_samples > 0 && num_rays > kMaxCount / num_samples))
        return snerf::fail(SNERF_E_UNSUPPORTED, "%s: num_rays . num_samples = %lld x %d exceeds 2^31 - 1", what, num_rays, num_samples);
    *total = num_rays * num_samples;
    return SNERF_OK;
}

}  // namespace

extern "C" int snerf_ray_samples_count(const float* weights, long long num_rays, int num_samples, double min_weight, int* offsets,
                                       snerf_stream_t stream) {
    long long total = 0;
    const int status = samples_extent("ray_samples_count", num_rays, num_samples, &total);
    if (status != SNERF_OK) return status;
    SNERF_REQUIRE(min_weight == min_weight, "ray_samples_count: min_weight is not a number");
    SNERF_REQUIRE(offsets && (total == 0 || weights), "ray_samples_count: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    // (without samples the rows are empty: every wave writes a zero)
    hipLaunchKernelGGL(ray_samples_count_kernel, dim3(blocks_of(num_rays + 1, kWaves)), dim3(kBlock), 0, s, weights, num_rays, num_samples,
                       min_weight, (uint32_t*)offsets);
    hipLaunchKernelGGL(scan_counters_kernel, dim3(1), dim3(kBlock), 0, s, (uint32_t*)offsets, num_rays + 1);
    return snerf::check_launch("ray_samples_count");
}

extern "C" int snerf_ray_samples_emit(const float* origins, const float* dirs, const float* z_vals, const float* weights,
                                      long long num_rays, int num_samples, double min_weight, const int* offsets, long long capacity,
                                      int* sample, float* points, snerf_stream_t stream) {
    long long total = 0;
    const int status = samples_extent("ray_samples_emit", num_rays, num_samples, &total);
    if (status != SNERF_OK) return status;
    SNERF_REQUIRE(min_weight == min_weight, "ray_samples_emit: min_weight is not a number");
    SNERF_REQUIRE(capacity >= 0, "ray_samples_emit: capacity %lld", capacity);
    SNERF_REQUIRE(offsets, "ray_samples_emit: offsets is NULL");
    if (total == 0 || capacity == 0) return SNERF_OK;
    SNERF_REQUIRE(origins && dirs && z_vals && weights && sample && points, "ray_samples_emit: NULL pointer");
    hipLaunchKernelGGL(ray_samples_emit_kernel, dim3(blocks_of(num_rays, kWaves)), dim3(kBlock), 0, (hipStream_t)stream, origins, dirs, z_vals,
                       weights, num_rays, num_samples, min_weight, offsets, capacity, sample, points);
    return snerf::check_launch("ray_samples_emit");
}

extern "C" int snerf_composite_normals(const float* points, const float* grad, long long count, const int* offsets, const int* sample,
                                       const float* weights, long long num_rays, int num_samples, int ndc, double cx, double cy,
                                       double near, float* normal, float* strength, snerf_stream_t stream) {
    long long total = 0;
    const int status = samples_extent("composite_normals", num_rays, num_samples, &total);
    if (status != SNERF_OK) return status;
    SNERF_REQUIRE(count >= 0, "composite_normals: count %lld", count);
    InputMap m;
    m.ndc = ndc ? 1 : 0;
    m.cx = m.cy = m.near = 0.0;
    if (ndc) {
        SNERF_REQUIRE(std::isfinite(cx) && std::isfinite(cy), "composite_normals: ndc parameters cx %g, cy %g are not finite", cx, cy);
        SNERF_REQUIRE(near > 0.0 && std::isfinite(near), "composite_normals: ndc near %g, expected a finite number > 0", near);
        m.cx = cx; m.cy = cy; m.near = near;
    }
    if (count > kMaxCount) return snerf::fail(SNERF_E_UNSUPPORTED, "composite_normals: count %lld exceeds 2^31 - 1", count);
    if (num_rays == 0) return SNERF_OK;
    SNERF_REQUIRE(offsets && normal && strength && (total == 0 || weights) && (count == 0 || (points && grad && sample)),
                  "composite_normals: NULL pointer");
    hipLaunchKernelGGL(composite_normals_kernel, dim3(blocks_of(num_rays, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, points, grad, count,
                       offsets, sample, weights, num_rays, total, m, normal, strength);
    return snerf::check_launch("composite_normals");
}

extern "C" int snerf_depth_normals(const float* depth, const unsigned char* mask, const double* cameras, int views, int height, int width,
                                   double edge_threshold, float* normals, snerf_stream_t stream) {
    SNERF_REQUIRE(views >= 0 && height >= 0 && width >= 0, "depth_normals: %d views of %d x %d", views, height, width);
    SNERF_REQUIRE(views <= SNERF_FUSE_MAX_VIEWS, "depth_normals: %d views, at most %d", views, SNERF_FUSE_MAX_VIEWS);
    SNERF_REQUIRE(edge_threshold == edge_threshold, "depth_normals: edge_threshold is not a number");
    const long long pixels = (long long)height * width;     // (< 2^62)
    if (views > 0 && pixels > kMaxCount / views)
        return snerf::fail(SNERF_E_UNSUPPORTED, "depth_normals: %d views of %d x %d exceed 2^31 - 1 pixels", views, height, width);
    DepthFrames f;
    f.depth = depth; f.mask = mask; f.cameras = cameras;
    f.views = views; f.height = height; f.width = width;
    f.pixels = pixels;
    f.total = pixels * views;
    if (f.total == 0) return SNERF_OK;
    SNERF_REQUIRE(depth && cameras && normals, "depth_normals: NULL pointer");
    hipLaunchKernelGGL(depth_normals_kernel, dim3(blocks_of(f.total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, f, edge_threshold, normals);
    return snerf::check_launch("depth_normals");
}

extern "C" int snerf_normals_to_u8(const float* normals, long long count, const double* rotation, unsigned char* image,
                                   snerf_stream_t stream) {
    SNERF_REQUIRE(count >= 0, "normals_to_u8: count %lld", count);
    Rotation R = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
    if (rotation) {
        for (int k = 0; k < 9; ++k) {
            SNERF_REQUIRE(std::isfinite(rotation[k]), "normals_to_u8: rotation[%d] = %g is not finite", k, rotation[k]);
            R.r[k] = rotation[k];
        }
    }
    if (count > kMaxCount) return snerf::fail(SNERF_E_UNSUPPORTED, "normals_to_u8: count %lld exceeds 2^31 - 1", count);
    if (count == 0) return SNERF_OK;
    SNERF_REQUIRE(normals && image, "normals_to_u8: NULL pointer");
    hipLaunchKernelGGL(normals_to_u8_kernel, dim3(blocks_of(count, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, normals, count, R, image);
    return snerf::check_launch("normals_to_u8");
}
