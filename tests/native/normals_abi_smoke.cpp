// The normal maps from the C ABI alone: plain HIP runtime + include/simplenerf_hip.h + csrc/simplenerf_normals.h, linked against
// libsimplenerf_hip.so, no PyTorch in the process.
//
//   normals_abi_smoke <fixture file>
//
// The fixture (tests/test_normals_host.py: native_fixture) holds rays, sample depths and weights, the restatement's selection of
// them, gradients at the selected points, the restatement's composited normals (with the NDC pull-back), depth maps with holes and
// their cameras, the restatement's depth normals, and the picture of the composited normals.  snerf_ray_samples_count +
// snerf_ray_samples_emit must give the offsets, the indices and the points exactly, snerf_composite_normals and
// snerf_depth_normals the restatement to one float32 ulp with zeros where it has zeros, snerf_normals_to_u8 the picture exactly;
// a second call gives the same bytes; the refusals are status codes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simplenerf_hip.h"
#include "simplenerf_normals.h"

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

template <typename T>
static hipError_t download(const T* device, std::vector<T>& host) {
    return hipMemcpy(host.data(), device, host.size() * sizeof(T), hipMemcpyDeviceToHost);
}

// the largest distance in float32 ulps between got and want (-1: a zero against a non-zero, another sign, or not a number)
static long long worst_ulps(const std::vector<float>& got, const std::vector<float>& want) {
    long long worst = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        if (got[i] == want[i]) continue;
        if (!(std::isfinite(got[i]) && std::isfinite(want[i])) || got[i] == 0.f || want[i] == 0.f || (got[i] < 0.f) != (want[i] < 0.f)) return -1;
        int32_t a, b;
        std::memcpy(&a, &got[i], 4);
        std::memcpy(&b, &want[i], 4);
        const long long d = std::llabs((long long)a - (long long)b);
        worst = d > worst ? d : worst;
    }
    return worst;
}

int main(int argc, char** argv) {
    if (argc != 2) return std::printf("usage: normals_abi_smoke fixture\n"), 1;
    CHECK(snerf_abi_version() == SNERF_ABI_VERSION);
    Reader in;
    CHECK(read_file(argv[1], in.bytes));
    const int rays = in.one<int32_t>(), samples = in.one<int32_t>(), count = in.one<int32_t>();
    const int views = in.one<int32_t>(), height = in.one<int32_t>(), width = in.one<int32_t>();
    const double min_weight = in.one<double>(), cx = in.one<double>(), cy = in.one<double>(), near_plane = in.one<double>();
    const double edge = in.one<double>();
    const std::vector<double> rotation = in.many<double>(9);
    CHECK(in.ok && rays >= 1 && rays <= 4096 && samples >= 1 && samples <= 4096 && count >= 1 && count <= rays * samples);
    CHECK(views >= 1 && views <= SNERF_FUSE_MAX_VIEWS && height >= 1 && height <= 1024 && width >= 1 && width <= 1024 && near_plane > 0.0);
    const size_t total = (size_t)rays * samples, pixels = (size_t)views * height * width;
    const std::vector<float> origins = in.many<float>((size_t)rays * 3), dirs = in.many<float>((size_t)rays * 3);
    const std::vector<float> z_vals = in.many<float>(total), weights = in.many<float>(total);
    const std::vector<int32_t> want_offsets = in.many<int32_t>((size_t)rays + 1), want_sample = in.many<int32_t>((size_t)count);
    const std::vector<float> want_points = in.many<float>((size_t)count * 3), grad = in.many<float>((size_t)count * 3);
    const std::vector<float> want_normal = in.many<float>((size_t)rays * 3), want_strength = in.many<float>((size_t)rays);
    const std::vector<double> cameras = in.many<double>((size_t)views * SNERF_FUSE_CAMERA_DOUBLES);
    const std::vector<float> depth = in.many<float>(pixels);
    const std::vector<unsigned char> mask = in.many<unsigned char>(pixels);
    const std::vector<float> want_depth_normals = in.many<float>(pixels * 3);
    const std::vector<unsigned char> want_image = in.many<unsigned char>((size_t)rays * 3);
    CHECK(in.ok && in.at == in.bytes.size());

    // ---- the selection: count, read M back, emit
    float *d_origins = nullptr, *d_dirs = nullptr, *d_z = nullptr, *d_weights = nullptr, *d_points = nullptr, *d_grad = nullptr;
    float *d_normal = nullptr, *d_strength = nullptr, *d_depth = nullptr, *d_depth_normals = nullptr, *d_want_normal = nullptr;
    int32_t *d_offsets = nullptr, *d_sample = nullptr;
    double* d_cameras = nullptr;
    unsigned char *d_mask = nullptr, *d_image = nullptr;
    HIP_OK(upload(origins, &d_origins));
    HIP_OK(upload(dirs, &d_dirs));
    HIP_OK(upload(z_vals, &d_z));
    HIP_OK(upload(weights, &d_weights));
    HIP_OK(hipMalloc((void**)&d_offsets, ((size_t)rays + 2) * 4));
    HIP_OK(hipMemset(d_offsets, 0xAA, ((size_t)rays + 2) * 4));
    CHECK(snerf_ray_samples_count(d_weights, -1, samples, min_weight, d_offsets, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_ray_samples_count(d_weights, rays, samples, (double)NAN, d_offsets, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_ray_samples_count(d_weights, rays, samples, min_weight, nullptr, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_ray_samples_count(d_weights, 1LL << 20, 1 << 11, min_weight, d_offsets, nullptr) == SNERF_E_UNSUPPORTED);
    CHECK(std::strstr(snerf_last_error(), "num_rays . num_samples") != nullptr);
    SNERF_OK_(snerf_ray_samples_count(d_weights, rays, samples, min_weight, d_offsets, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<int32_t> offsets((size_t)rays + 2);
    HIP_OK(download(d_offsets, offsets));
    CHECK((uint32_t)offsets[(size_t)rays + 1] == 0xAAAAAAAAu);          // the slot past the total is not written
    CHECK(std::memcmp(offsets.data(), want_offsets.data(), ((size_t)rays + 1) * 4) == 0);
    const long long selected = offsets[(size_t)rays];
    CHECK(selected == count);
    HIP_OK(hipMalloc((void**)&d_sample, ((size_t)count + 1) * 4));
    HIP_OK(hipMalloc((void**)&d_points, ((size_t)count + 1) * 12));
    HIP_OK(hipMemset(d_sample, 0xAA, ((size_t)count + 1) * 4));
    HIP_OK(hipMemset(d_points, 0xAA, ((size_t)count + 1) * 12));
    auto emit = [&](long long capacity, int32_t* sample, float* points) {
        return snerf_ray_samples_emit(d_origins, d_dirs, d_z, d_weights, rays, samples, min_weight, d_offsets, capacity, sample, points, nullptr);
    };
    CHECK(emit(-1, d_sample, d_points) == SNERF_E_INVALID);
    CHECK(emit(count, nullptr, d_points) == SNERF_E_INVALID);
    SNERF_OK_(emit(0, nullptr, nullptr));
    SNERF_OK_(emit(count, d_sample, d_points));
    HIP_OK(hipDeviceSynchronize());
    std::vector<int32_t> sample((size_t)count + 1);
    std::vector<float> points(((size_t)count + 1) * 3);
    HIP_OK(download(d_sample, sample));
    HIP_OK(download(d_points, points));
    CHECK((uint32_t)sample[(size_t)count] == 0xAAAAAAAAu);               // rows past the capacity are not written
    CHECK(std::memcmp(sample.data(), want_sample.data(), (size_t)count * 4) == 0);
    CHECK(std::memcmp(points.data(), want_points.data(), (size_t)count * 12) == 0);
    {   // a capacity below M: the rows that fit are written, none past them
        HIP_OK(hipMemset(d_sample, 0xAA, ((size_t)count + 1) * 4));
        SNERF_OK_(emit(count / 2, d_sample, d_points));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(download(d_sample, sample));
        CHECK(std::memcmp(sample.data(), want_sample.data(), (size_t)(count / 2) * 4) == 0);
        for (int k = count / 2; k <= count; ++k) CHECK((uint32_t)sample[(size_t)k] == 0xAAAAAAAAu);
        SNERF_OK_(emit(count, d_sample, d_points));
    }

    // ---- the compositing, with the NDC pull-back
    HIP_OK(upload(grad, &d_grad));
    HIP_OK(hipMalloc((void**)&d_normal, (size_t)rays * 12));
    HIP_OK(hipMalloc((void**)&d_strength, (size_t)rays * 4));
    auto composite = [&](long long n, int ndc, double near, float* normal) {
        return snerf_composite_normals(d_points, d_grad, n, d_offsets, d_sample, d_weights, rays, samples, ndc, cx, cy, near, normal, d_strength,
                                       nullptr);
    };
    CHECK(composite(-1, 1, near_plane, d_normal) == SNERF_E_INVALID);
    CHECK(composite(count, 1, 0.0, d_normal) == SNERF_E_INVALID);
    CHECK(composite(count, 1, near_plane, nullptr) == SNERF_E_INVALID);
    CHECK(composite(1LL << 31, 1, near_plane, d_normal) == SNERF_E_UNSUPPORTED);
    SNERF_OK_(composite(count, 1, near_plane, d_normal));
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> normal((size_t)rays * 3), strength((size_t)rays), again((size_t)rays * 3);
    HIP_OK(download(d_normal, normal));
    HIP_OK(download(d_strength, strength));
    const long long normal_ulps = worst_ulps(normal, want_normal), strength_ulps = worst_ulps(strength, want_strength);
    int empty = 0;
    for (int r = 0; r < rays; ++r) empty += want_strength[(size_t)r] == 0.f;
    std::printf("normals_abi_smoke: %d rays of %d samples, %d selected, %d rays without a normal, worst difference %lld ulp [1] (strength %lld [1])\n",
                rays, samples, count, empty, normal_ulps, strength_ulps);
    CHECK(normal_ulps >= 0 && normal_ulps <= 1 && strength_ulps >= 0 && strength_ulps <= 1 && empty > 0 && empty < rays);
    SNERF_OK_(composite(count, 1, near_plane, d_normal));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(download(d_normal, again));
    CHECK(std::memcmp(again.data(), normal.data(), again.size() * 4) == 0);

    // ---- the depth normals
    HIP_OK(upload(depth, &d_depth));
    HIP_OK(upload(mask, &d_mask));
    HIP_OK(upload(cameras, &d_cameras));
    HIP_OK(hipMalloc((void**)&d_depth_normals, (pixels + 1) * 12));
    HIP_OK(hipMemset(d_depth_normals, 0xAA, (pixels + 1) * 12));
    CHECK(snerf_depth_normals(d_depth, d_mask, d_cameras, -1, height, width, edge, d_depth_normals, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_depth_normals(d_depth, d_mask, nullptr, views, height, width, edge, d_depth_normals, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_depth_normals(d_depth, d_mask, d_cameras, views, height, width, (double)NAN, d_depth_normals, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_depth_normals(d_depth, d_mask, d_cameras, 2, 1 << 16, 1 << 15, edge, d_depth_normals, nullptr) == SNERF_E_UNSUPPORTED);
    SNERF_OK_(snerf_depth_normals(d_depth, d_mask, d_cameras, views, height, width, edge, d_depth_normals, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> depth_normals((pixels + 1) * 3);
    HIP_OK(download(d_depth_normals, depth_normals));
    uint32_t bits;
    std::memcpy(&bits, &depth_normals[pixels * 3], 4);
    CHECK(bits == 0xAAAAAAAAu);
    depth_normals.resize(pixels * 3);
    const long long depth_ulps = worst_ulps(depth_normals, want_depth_normals);
    size_t flat = 0;
    for (size_t i = 0; i < pixels; ++i) flat += want_depth_normals[3 * i] == 0.f && want_depth_normals[3 * i + 1] == 0.f && want_depth_normals[3 * i + 2] == 0.f;
    std::printf("normals_abi_smoke: %d views of %d x %d, %zu pixels without a normal, worst difference %lld ulp [1]\n", views, height, width,
                flat, depth_ulps);
    CHECK(depth_ulps >= 0 && depth_ulps <= 1 && flat > 0 && flat < pixels);

    // ---- the picture, of the restatement's normals so that it is exact
    HIP_OK(upload(want_normal, &d_want_normal));
    HIP_OK(hipMalloc((void**)&d_image, (size_t)rays * 3 + 1));
    HIP_OK(hipMemset(d_image, 0x55, (size_t)rays * 3 + 1));
    std::vector<double> bad = rotation;
    bad[4] = (double)INFINITY;
    CHECK(snerf_normals_to_u8(d_want_normal, rays, bad.data(), d_image, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_normals_to_u8(d_want_normal, -1, rotation.data(), d_image, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_normals_to_u8(d_want_normal, rays, rotation.data(), nullptr, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_normals_to_u8(nullptr, 0, nullptr, nullptr, nullptr) == SNERF_OK);
    SNERF_OK_(snerf_normals_to_u8(d_want_normal, rays, rotation.data(), d_image, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<unsigned char> image((size_t)rays * 3 + 1);
    HIP_OK(download(d_image, image));
    int differing = 0;
    for (size_t i = 0; i < want_image.size(); ++i) differing += image[i] != want_image[i];
    std::printf("normals_abi_smoke: picture of %d normals, %d bytes differ [0]\n", rays, differing);
    CHECK(differing == 0 && image[(size_t)rays * 3] == 0x55);

    for (float* p : {d_origins, d_dirs, d_z, d_weights, d_points, d_grad, d_normal, d_strength, d_depth, d_depth_normals, d_want_normal})
        HIP_OK(hipFree(p));
    HIP_OK(hipFree(d_offsets));
    HIP_OK(hipFree(d_sample));
    HIP_OK(hipFree(d_cameras));
    HIP_OK(hipFree(d_mask));
    HIP_OK(hipFree(d_image));
    std::printf("normals_abi_smoke: OK\n");
    return 0;
}
