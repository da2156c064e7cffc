// The scene tables from the C ABI alone: plain HIP runtime + include/simplenerf_train.h, linked against libsimplenerf_hip.so, no torch
// in the process.  Two 11 x 13 views with RGBA images and sparse-depth points built from integer expressions (shared pixels, half-way
// coordinates, points outside the frame, a view without points): snerf_scene_images, snerf_rasterise_sparse_depth (with its NDC
// table) and snerf_depth_table_to_ndc are compared, bit for bit, with the same rules written out here -- the last point in input order
// wins a pixel; with an identity pose every ray has oz = 0 and dz = -1, so the NDC depth needs no camera arithmetic on the host.
// Built and run by tests/test_gpu_scene_native.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simplenerf_train.h"

#define SNERF_OK_(x)                                                                   \
    do {                                                                               \
        if ((x) != 0) { std::printf("ABI error at %s:%d: %s\n", __FILE__, __LINE__, snerf_last_error()); return 3; } \
    } while (0)
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::printf("check failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); return 4; } \
    } while (0)

template <typename T>
static T* dev(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) std::abort();
    return static_cast<T*>(p);
}
template <typename T>
static T* upload(const std::vector<T>& h) {
    T* d = dev<T>(h.size());
    if (h.size() && hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) std::abort();
    return d;
}
template <typename T>
static std::vector<T> host(const T* d, size_t n) {
    std::vector<T> h(n);
    if (n && hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) std::abort();
    return h;
}
static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

// convert_depth_to_ndc for a ray with oz = 0, dz = -1, in float, in the library's order
static float ndc_of(float depth, float near) {
    const float oz = 0.0f, dz = -1.0f;
    const float tn = -(near + oz) / dz;
    const float oz_prime = oz + tn * dz;
    const float ndc = 1.0f - oz_prime / (oz_prime + (depth - tn) * dz);
    return depth == -1.0f ? -1.0f : ndc;
}

int main() {
    CHECK(snerf_abi_version() == SNERF_ABI_VERSION);
    const int views = 3, h = 11, w = 13;
    const long long pixels = (long long)views * h * w;

    // S1: RGBA on a white background, and plain RGB
    std::vector<unsigned char> rgba(pixels * 4);
    for (size_t i = 0; i < rgba.size(); ++i) rgba[i] = (unsigned char)((i * 37 + (i / 4) * 11) % 256);
    unsigned char* d_rgba = upload(rgba);
    float* d_images = dev<float>(pixels * 3);
    for (int white = 0; white < 2; ++white) {
        SNERF_OK_(snerf_scene_images(d_rgba, pixels, 4, white, d_images, nullptr));
        if (hipDeviceSynchronize() != hipSuccess) return 2;
        std::vector<float> want(pixels * 3);
        for (long long i = 0; i < pixels; ++i) {
            const float a = (float)rgba[4 * i + 3] / 255.0f, rest = 1.0f - a;
            for (int c = 0; c < 3; ++c) {
                const float v = (float)rgba[4 * i + c] / 255.0f;
                want[3 * i + c] = white ? v * a + rest : v;
            }
        }
        CHECK(same_bits(host(d_images, pixels * 3), want));
    }

    // S2: points of views 0 and 2 (view 1 has none); every third point repeats an earlier pixel, some lie outside the frame
    std::vector<double> x, y, depth, error;
    std::vector<int> view;
    for (int v = 0; v < views; v += 2)
        for (int k = 0; k < 60; ++k) {
            x.push_back(k % 3 == 2 ? x[x.size() - 2] + 0.25 : ((k * 7) % (w + 6)) - 3 + 0.5 * (k % 2));       // -3 .. w+2, halves
            y.push_back(k % 3 == 2 ? y[y.size() - 2] - 0.25 : ((k * 5) % (h + 4)) - 2 + 0.5 * ((k / 2) % 2));
            depth.push_back(2.0 + 0.125 * k + v);
            error.push_back(0.5 + 0.0625 * k);
            view.push_back(v);
        }
    const long long points = (long long)x.size();
    const double scale = 0.625, divisor = 1.0;
    const float near = 1.0f;
    std::vector<float> want_depths(pixels, -1.0f), want_errors(pixels, -1.0f), want_ndc(pixels);
    for (long long p = 0; p < points; ++p) {          // input order: a later point overwrites an earlier one
        const int px = (int)std::fmin(std::fmax(std::nearbyint(x[p] / divisor), 0.0), (double)(w - 1));
        const int py = (int)std::fmin(std::fmax(std::nearbyint(y[p] / divisor), 0.0), (double)(h - 1));
        const long long i = ((long long)view[p] * h + py) * w + px;
        want_depths[i] = (float)(depth[p] * scale);
        want_errors[i] = (float)error[p];
    }
    for (long long i = 0; i < pixels; ++i) want_ndc[i] = ndc_of(want_depths[i], near);

    std::vector<float> intrinsics, poses;
    for (int v = 0; v < views; ++v) {
        const float k[9] = {12.0f + v, 0, 6.5f, 0, 12.0f + v, 5.5f, 0, 0, 1};
        intrinsics.insert(intrinsics.end(), k, k + 9);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) poses.push_back(r == c ? 1.0f : (c == 3 && r < 2 ? 0.25f * (v + 1) : 0.0f));   // oz stays 0
    }
    float *d_intrinsics = upload(intrinsics), *d_poses = upload(poses), *d_table = dev<float>(views * SNERF_CAMERA_FLOATS);
    SNERF_OK_(snerf_camera_table(d_intrinsics, d_poses, views, h, w, d_table, nullptr));
    double *d_x = upload(x), *d_y = upload(y), *d_depth = upload(depth), *d_error = upload(error);
    int* d_view = upload(view);
    const long long ws_bytes = snerf_rasterise_sparse_depth_workspace_bytes(views, h, w);
    CHECK(ws_bytes == pixels * (long long)sizeof(int));
    void* ws = dev<char>((size_t)ws_bytes);
    float *d_depths = dev<float>(pixels), *d_errors = dev<float>(pixels), *d_ndc = dev<float>(pixels), *d_ndc2 = dev<float>(pixels);
    for (int run = 0; run < 2; ++run) {                // twice: the same bits
        SNERF_OK_(snerf_rasterise_sparse_depth(d_x, d_y, d_depth, d_error, d_view, points, scale, divisor, d_table, near, views, h, w,
                                               d_depths, d_errors, d_ndc, ws, nullptr));
        SNERF_OK_(snerf_depth_table_to_ndc(d_depths, d_table, views, h, w, near, d_ndc2, nullptr));
        if (hipDeviceSynchronize() != hipSuccess) return 2;
        CHECK(same_bits(host(d_depths, pixels), want_depths));
        CHECK(same_bits(host(d_errors, pixels), want_errors));
        CHECK(same_bits(host(d_ndc, pixels), want_ndc));
        CHECK(same_bits(host(d_ndc2, pixels), want_ndc));
    }
    long long filled = 0;
    for (long long i = 0; i < pixels; ++i) filled += want_depths[i] != -1.0f;
    CHECK(filled > 40 && filled < points);             // shared pixels exist
    for (long long i = (long long)h * w; i < 2LL * h * w; ++i) CHECK(want_depths[i] == -1.0f && want_ndc[i] == -1.0f);   // view 1

    // no points: tables of -1; bad arguments: refused with a message
    SNERF_OK_(snerf_rasterise_sparse_depth(nullptr, nullptr, nullptr, nullptr, nullptr, 0, scale, divisor, d_table, near, views, h, w,
                                           d_depths, d_errors, d_ndc, ws, nullptr));
    if (hipDeviceSynchronize() != hipSuccess) return 2;
    CHECK(same_bits(host(d_depths, pixels), std::vector<float>(pixels, -1.0f)));
    CHECK(same_bits(host(d_ndc, pixels), std::vector<float>(pixels, -1.0f)));
    CHECK(snerf_rasterise_sparse_depth(d_x, d_y, d_depth, d_error, nullptr, points, scale, divisor, d_table, near, views, h, w, d_depths,
                                       d_errors, d_ndc, ws, nullptr) < 0 && std::strstr(snerf_last_error(), "NULL"));
    CHECK(snerf_rasterise_sparse_depth(d_x, d_y, d_depth, d_error, d_view, 1LL << 31, scale, divisor, d_table, near, views, h, w, d_depths,
                                       d_errors, d_ndc, ws, nullptr) < 0 && std::strstr(snerf_last_error(), "2^31-1"));
    CHECK(snerf_scene_images(d_rgba, pixels, 2, 0, d_images, nullptr) < 0);
    std::printf("scene_abi_smoke: OK (%lld points on %lld of %lld pixels)\n", points, filled, pixels);
    return 0;
}
