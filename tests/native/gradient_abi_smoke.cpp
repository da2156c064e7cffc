// The field's gradient and its normals from the C ABI alone: plain HIP runtime + include/simplenerf_hip.h +
// csrc/simplenerf_gradient.h, linked against libsimplenerf_hip.so, no PyTorch in the process.
//
//   gradient_abi_smoke <fixture file>
//
// The fixture (tests/test_field_gradient_host.py: native_fixture) holds points, the float64 oracle's density gradient at them, which
// of them may be compared and at what tolerance, NDC parameters, and the seeded 8 x 128 / 64 MLP.  snerf_mlp_pack_for (fp32,
// training) + snerf_mlp_forward_train (every point a ray of one sample at depth 0) + snerf_mlp_input_gradient must give that
// gradient, exact zeros where the density is 0, and the same bytes on a second call; snerf_field_normals turns it into unit
// normals, with and without the NDC pull-back; the refusals are status codes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simplenerf_hip.h"
#include "simplenerf_gradient.h"

#define HIP_OK(x)                                                                      \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) { std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 2; } \
    } while (0)
#define SNERF_OK_(x)                                                                   \
    do {                                                                               \
        if ((x) != 0) { std::printf("ABI error at %s:%d: %s\n", __FILE__, __LINE__, snerf_last_error()); return 3; } \
    } while (0)
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::printf("check failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); return 4; } \
    } while (0)

struct Reader {
    std::vector<unsigned char> bytes;
    size_t at = 0;
    bool ok = true;
    template <typename T>
    T one() {
        T value{};
        if (at + sizeof(T) > bytes.size()) { ok = false; return value; }
        std::memcpy(&value, bytes.data() + at, sizeof(T));
        at += sizeof(T);
        return value;
    }
    template <typename T>
    std::vector<T> many(size_t count) {
        std::vector<T> values;
        if (count > (bytes.size() - at) / sizeof(T)) { ok = false; return values; }
        values.resize(count);
        if (count) std::memcpy(values.data(), bytes.data() + at, count * sizeof(T));
        at += count * sizeof(T);
        return values;
    }
};

static bool read_file(const char* path, std::vector<unsigned char>& bytes) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    bytes.resize(size > 0 ? (size_t)size : 0);
    const bool ok = std::fread(bytes.data(), 1, bytes.size(), f) == bytes.size();
    std::fclose(f);
    return ok;
}

template <typename T>
static hipError_t upload(const std::vector<T>& host, T** device) {
    hipError_t e = hipMalloc((void**)device, host.size() * sizeof(T) + 16);
    if (e != hipSuccess) return e;
    return hipMemcpy(*device, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
}

int main(int argc, char** argv) {
    if (argc != 2) return std::printf("usage: gradient_abi_smoke fixture\n"), 1;
    CHECK(snerf_abi_version() == SNERF_ABI_VERSION);
    Reader in;
    CHECK(read_file(argv[1], in.bytes));
    const int count = in.one<int32_t>(), np = in.one<int32_t>();
    const double cx = in.one<double>(), cy = in.one<double>(), near_plane = in.one<double>();
    CHECK(in.ok && count >= 1 && count <= (1 << 16) && near_plane > 0.0);
    const std::vector<float> points = in.many<float>((size_t)count * 3), want = in.many<float>((size_t)count * 3);
    const std::vector<unsigned char> compared = in.many<unsigned char>((size_t)count);
    const float tolerance = in.one<float>();
    snerf_mlp_desc desc = {8, 128, 1, 64, 10, 4, -1, 1, 1};
    CHECK(in.ok && tolerance > 0.f && np == snerf_mlp_num_params(&desc) && np == 24);
    std::vector<float*> params(np, nullptr);
    for (int i = 0; i < np; ++i) {
        const long long floats = in.one<int64_t>();
        CHECK(in.ok && floats >= 1 && floats <= (1 << 20));
        const std::vector<float> values = in.many<float>((size_t)floats);
        CHECK(in.ok);
        HIP_OK(upload(values, &params[i]));
    }
    CHECK(in.at == in.bytes.size());

    // ---- the storing forward: every point a ray of one sample, origin = the point, direction and depth 0
    float *d_packed = nullptr, *d_points = nullptr, *d_zero = nullptr, *d_dirs = nullptr, *d_sigma = nullptr, *d_rgb = nullptr;
    float *d_saved = nullptr, *d_ones = nullptr, *d_work = nullptr, *d_grad = nullptr, *d_normals = nullptr;
    const size_t packed_bytes = snerf_mlp_packed_floats(&desc) * sizeof(float);
    HIP_OK(hipMalloc((void**)&d_packed, packed_bytes));
    HIP_OK(hipMemset(d_packed, 0, packed_bytes));
    SNERF_OK_(snerf_mlp_pack_for(&desc, params.data(), np, d_packed, SNERF_PRECISION_FP32, 1, nullptr));
    HIP_OK(upload(points, &d_points));
    std::vector<float> down((size_t)count * 3, 0.f), ones((size_t)count, 1.f);
    for (int n = 0; n < count; ++n) down[3 * n + 2] = -1.f;
    HIP_OK(upload(down, &d_dirs));
    HIP_OK(upload(ones, &d_ones));
    HIP_OK(hipMalloc((void**)&d_zero, (size_t)count * 3 * sizeof(float)));
    HIP_OK(hipMemset(d_zero, 0, (size_t)count * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_sigma, (size_t)count * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_rgb, (size_t)count * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_saved, snerf_mlp_saved_floats(&desc, count, 1) * sizeof(float)));
    SNERF_OK_(snerf_mlp_forward_train(&desc, d_packed, d_points, d_zero, d_dirs, d_zero, count, 1, nullptr, d_sigma, d_rgb, d_saved,
                                      SNERF_PRECISION_FP32, nullptr));

    // ---- the gradient; every refusal comes before the first launch
    const size_t work_floats = snerf_mlp_input_gradient_workspace_floats(&desc, count);
    CHECK(work_floats > 0 && snerf_mlp_input_gradient_workspace_floats(&desc, 0) == 0);
    HIP_OK(hipMalloc((void**)&d_work, work_floats * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_grad, (size_t)(count + 1) * 3 * sizeof(float)));
    HIP_OK(hipMemset(d_grad, 0xAA, (size_t)(count + 1) * 3 * sizeof(float)));
    auto gradient = [&](const snerf_mlp_desc* which, const float* packed, int num_params, long long n, float* out) {
        return snerf_mlp_input_gradient(which, packed, params.data(), num_params, d_saved, d_sigma, d_ones, n, d_work, out, nullptr);
    };
    snerf_mlp_desc visible = desc, layered = desc;
    visible.predict_visibility = 1;
    layered.points_net_width = 96;
    layered.views_net_width = 48;
    CHECK(gradient(&visible, d_packed, np, count, d_grad) == SNERF_E_UNSUPPORTED);
    CHECK(std::strstr(snerf_last_error(), "predict_visibility") != nullptr);
    CHECK(gradient(&layered, d_packed, np, count, d_grad) == SNERF_E_UNSUPPORTED);
    CHECK(std::strstr(snerf_last_error(), "layered") != nullptr);
    CHECK(snerf_mlp_input_gradient_workspace_floats(&visible, count) == 0 && snerf_mlp_input_gradient_workspace_floats(&layered, count) == 0);
    CHECK(gradient(&desc, d_packed, np, 0, d_grad) == SNERF_E_INVALID);
    CHECK(gradient(&desc, d_packed, np - 1, count, d_grad) == SNERF_E_INVALID);
    CHECK(gradient(&desc, d_packed, np, count, nullptr) == SNERF_E_INVALID);
    CHECK(gradient(&desc, nullptr, np, count, d_grad) == SNERF_E_INVALID);
    {   // a stream packed for rendering only does not hold the transposed weights the chain reads
        float* d_render = nullptr;
        HIP_OK(hipMalloc((void**)&d_render, packed_bytes));
        HIP_OK(hipMemset(d_render, 0, packed_bytes));
        SNERF_OK_(snerf_mlp_pack_for(&desc, params.data(), np, d_render, SNERF_PRECISION_BF16, 0, nullptr));
        CHECK(gradient(&desc, d_render, np, count, d_grad) == SNERF_E_INVALID);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(d_render));
    }
    SNERF_OK_(gradient(&desc, d_packed, np, count, d_grad));
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> grad((size_t)(count + 1) * 3), again((size_t)count * 3), sigma((size_t)count);
    HIP_OK(hipMemcpy(grad.data(), d_grad, grad.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(sigma.data(), d_sigma, sigma.size() * sizeof(float), hipMemcpyDeviceToHost));
    uint32_t bits;     // rows past the count are not written
    std::memcpy(&bits, &grad[3 * (size_t)count], 4);
    CHECK(bits == 0xAAAAAAAAu);
    int checked = 0, closed = 0;
    float worst = 0.f;
    for (int n = 0; n < count; ++n) {
        for (int a = 0; a < 3; ++a) {
            const float g = grad[3 * n + a];
            CHECK(std::isfinite(g));
            if (sigma[n] == 0.f) CHECK(g == 0.f);
            if (compared[n]) worst = std::fmax(worst, std::fabs(g - want[3 * n + a]));
        }
        checked += compared[n] != 0;
        closed += sigma[n] == 0.f;
    }
    std::printf("gradient_abi_smoke: %d points, %d compared, %d closed, worst difference %.3e [%.3e]\n", count, checked, closed, worst, tolerance);
    CHECK(checked > 0 && worst <= tolerance);
    SNERF_OK_(gradient(&desc, d_packed, np, count, d_grad));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(again.data(), d_grad, again.size() * sizeof(float), hipMemcpyDeviceToHost));
    CHECK(std::memcmp(again.data(), grad.data(), again.size() * sizeof(float)) == 0);

    // ---- the normals: the points read as scene points; with ndc they are pushed behind the near plane first
    HIP_OK(hipMalloc((void**)&d_normals, (size_t)count * 3 * sizeof(float)));
    CHECK(snerf_field_normals(d_points, d_grad, -1, 0, 0.0, 0.0, 0.0, d_normals, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_field_normals(d_points, d_grad, count, 1, cx, cy, 0.0, d_normals, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_field_normals(d_points, d_grad, count, 1, (double)NAN, cy, near_plane, d_normals, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_field_normals(d_points, nullptr, count, 0, 0.0, 0.0, 0.0, d_normals, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_field_normals(d_points, d_grad, 1LL << 31, 0, 0.0, 0.0, 0.0, d_normals, nullptr) == SNERF_E_UNSUPPORTED);
    CHECK(snerf_field_normals(nullptr, nullptr, 0, 0, 0.0, 0.0, 0.0, nullptr, nullptr) == SNERF_OK);
    std::vector<float> normals((size_t)count * 3);
    for (int ndc = 0; ndc < 2; ++ndc) {
        std::vector<float> scene = points;
        if (ndc)
            for (int n = 0; n < count; ++n) scene[3 * n + 2] = (float)(-near_plane - 0.5 - std::fabs(points[3 * n + 2]));
        float* d_scene = nullptr;
        HIP_OK(upload(scene, &d_scene));
        SNERF_OK_(snerf_field_normals(d_scene, d_grad, count, ndc, cx, cy, near_plane, d_normals, nullptr));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(normals.data(), d_normals, normals.size() * sizeof(float), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_scene));
        for (int n = 0; n < count; ++n) {
            double norm = 0.0, G[3] = {grad[3 * n], grad[3 * n + 1], grad[3 * n + 2]}, along = 0.0;
            if (ndc) {
                const double x = scene[3 * n], y = scene[3 * n + 1], z = scene[3 * n + 2], g[3] = {G[0], G[1], G[2]};
                G[0] = cx / z * g[0];
                G[1] = cy / z * g[1];
                G[2] = -(cx * x * g[0] + cy * y * g[1] + 2.0 * near_plane * g[2]) / (z * z);
            }
            for (int a = 0; a < 3; ++a) {
                norm += (double)normals[3 * n + a] * normals[3 * n + a];
                along += (double)normals[3 * n + a] * G[a];
            }
            const double length = std::sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2]);
            if (sigma[n] == 0.f) {
                CHECK(norm == 0.0);
            } else {
                CHECK(std::fabs(norm - 1.0) < 1e-6 && std::fabs(along + length) <= 1e-6 * length);     // unit, and along -G
            }
        }
    }
    for (float* p : params) HIP_OK(hipFree(p));
    for (float* p : {d_packed, d_points, d_zero, d_dirs, d_sigma, d_rgb, d_saved, d_ones, d_work, d_grad, d_normals}) HIP_OK(hipFree(p));
    std::printf("gradient_abi_smoke: OK\n");
    return 0;
}
