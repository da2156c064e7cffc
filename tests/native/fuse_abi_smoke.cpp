// The point-cloud export from the C ABI alone: plain HIP runtime + include/simplenerf_hip.h + csrc/simplenerf_fuse.h, linked against
// libsimplenerf_hip.so, no PyTorch in the process.
//
//   fuse_abi_smoke <fixture file>
//
// The fixture (tests/fuse_reference.py: native_fixture) holds the analytic scene, the restated fuse of it and the restated thinning of
// those restated points.  snerf_fuse_depth_maps must give the fixture's N, its first and its last record (positions equal or adjacent
// floats, colours and view counts equal); snerf_voxel_thin on the fixture's points must give its M and its first and last run bit for
// bit; the refusals are status codes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simplenerf_hip.h"
#include "simplenerf_fuse.h"

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

// equal, or neighbours among the floats
static bool adjacent(float a, float b) { return a == b || std::nextafterf(a, b) == b; }

template <typename T>
static hipError_t upload(const std::vector<T>& host, T** device) {
    hipError_t e = hipMalloc((void**)device, host.size() * sizeof(T) + 16);
    if (e != hipSuccess) return e;
    return hipMemcpy(*device, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
}

int main(int argc, char** argv) {
    if (argc != 2) return std::printf("usage: fuse_abi_smoke fixture\n"), 1;
    CHECK(snerf_abi_version() == SNERF_ABI_VERSION);
    Reader in;
    CHECK(read_file(argv[1], in.bytes));
    const int views = in.one<int32_t>(), h = in.one<int32_t>(), w = in.one<int32_t>(), min_views = in.one<int32_t>();
    const double tau = in.one<double>();
    CHECK(in.ok && views >= 2 && views <= SNERF_FUSE_MAX_VIEWS && h >= 1 && w >= 1 && h <= 4096 && w <= 4096);
    const size_t total = (size_t)views * h * w;
    const std::vector<double> cameras = in.many<double>((size_t)views * SNERF_FUSE_CAMERA_DOUBLES);
    const std::vector<float> depth = in.many<float>(total);
    const std::vector<unsigned char> image = in.many<unsigned char>(total * 3);
    const long long n = in.one<int64_t>();
    CHECK(in.ok && n >= 1 && (size_t)n <= total);
    const std::vector<float> want_points = in.many<float>((size_t)n * 3);
    const std::vector<unsigned char> want_colours = in.many<unsigned char>((size_t)n * 3);
    const std::vector<unsigned char> want_views = in.many<unsigned char>((size_t)n);
    const double voxel_size = in.one<double>();
    double lo[3];
    for (double& v : lo) v = in.one<double>();
    int extents[3];
    for (int& v : extents) v = in.one<int32_t>();
    const long long m = in.one<int64_t>();
    CHECK(in.ok && m >= 1 && m <= n);
    const std::vector<float> want_thin = in.many<float>((size_t)m * 3);
    const std::vector<unsigned char> want_thin_colours = in.many<unsigned char>((size_t)m * 3);
    const std::vector<int32_t> want_counts = in.many<int32_t>((size_t)m);
    CHECK(in.ok && in.at == in.bytes.size());

    // ---- the fuse
    const long long fuse_bytes = snerf_fuse_depth_maps_workspace_bytes(views, h, w);
    CHECK(fuse_bytes >= (long long)total);
    CHECK(snerf_fuse_depth_maps_workspace_bytes(0, h, w) == 0 && snerf_fuse_depth_maps_workspace_bytes(views, -1, w) == 0 &&
          snerf_fuse_depth_maps_workspace_bytes(SNERF_FUSE_MAX_VIEWS + 1, h, w) == 0);
    double* d_cameras = nullptr;
    float *d_depth = nullptr, *d_points = nullptr;
    unsigned char *d_image = nullptr, *d_colours = nullptr, *d_views = nullptr;
    long long* d_count = nullptr;
    void* d_work = nullptr;
    HIP_OK(upload(cameras, &d_cameras));
    HIP_OK(upload(depth, &d_depth));
    HIP_OK(upload(image, &d_image));
    HIP_OK(hipMalloc((void**)&d_points, total * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_colours, total * 3));
    HIP_OK(hipMalloc((void**)&d_views, total));
    HIP_OK(hipMalloc((void**)&d_count, 2 * sizeof(long long)));
    HIP_OK(hipMalloc(&d_work, (size_t)fuse_bytes));
    HIP_OK(hipMemset(d_points, 0xAA, total * 3 * sizeof(float)));
    // every refusal comes before the first launch
    CHECK(snerf_fuse_depth_maps(d_depth, d_image, nullptr, d_cameras, views, h, w, -1.0, min_views, d_points, d_colours, d_views, d_count,
                                d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_fuse_depth_maps(d_depth, d_image, nullptr, d_cameras, views, h, w, tau, views, d_points, d_colours, d_views, d_count,
                                d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_fuse_depth_maps(nullptr, d_image, nullptr, d_cameras, views, h, w, tau, min_views, d_points, d_colours, d_views, d_count,
                                d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_fuse_depth_maps(d_depth, d_image, nullptr, d_cameras, views, h, w, tau, min_views, d_points, d_colours, d_views, d_count,
                                (char*)d_work + 8, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_fuse_depth_maps(nullptr, nullptr, nullptr, nullptr, views, 0, w, tau, min_views, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr) == SNERF_OK);     // (nothing to do: nothing enqueued)
    SNERF_OK_(snerf_fuse_depth_maps(d_depth, d_image, nullptr, d_cameras, views, h, w, tau, min_views, d_points, d_colours, d_views,
                                    d_count, d_work, nullptr));
    HIP_OK(hipDeviceSynchronize());
    long long got_n = -1;
    HIP_OK(hipMemcpy(&got_n, d_count, sizeof(long long), hipMemcpyDeviceToHost));
    std::printf("fuse_abi_smoke: fused %lld points of %zu pixels, expected %lld\n", got_n, total, n);
    CHECK(got_n == n);
    std::vector<float> points(total * 3);
    std::vector<unsigned char> colours(total * 3), agreeing(total);
    HIP_OK(hipMemcpy(points.data(), d_points, points.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(colours.data(), d_colours, colours.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(agreeing.data(), d_views, agreeing.size(), hipMemcpyDeviceToHost));
    for (long long record : {0LL, n - 1}) {
        for (int a = 0; a < 3; ++a) {
            CHECK(adjacent(points[3 * record + a], want_points[3 * record + a]));
            CHECK(colours[3 * record + a] == want_colours[3 * record + a]);
        }
        CHECK(agreeing[record] == want_views[record]);
    }
    if ((size_t)n < total) {     // rows past N are not written
        uint32_t bits;
        std::memcpy(&bits, &points[3 * n], 4);
        CHECK(bits == 0xAAAAAAAAu);
    }

    // ---- the thinning, of the fixture's own points
    const long long thin_bytes = snerf_voxel_thin_workspace_bytes(n, extents[0], extents[1], extents[2]);
    CHECK(thin_bytes > 0);
    CHECK(snerf_voxel_thin_workspace_bytes(n, 0, 1, 1) == 0 && snerf_voxel_thin_workspace_bytes(n, 65536, 65536, 1) == 0 &&
          snerf_voxel_thin_workspace_bytes(0, 1, 1, 1) == 0);
    float *d_in = nullptr, *d_thin = nullptr;
    unsigned char *d_in_colours = nullptr, *d_thin_colours = nullptr;
    int* d_counts = nullptr;
    void* d_thin_work = nullptr;
    HIP_OK(upload(want_points, &d_in));
    HIP_OK(upload(want_colours, &d_in_colours));
    HIP_OK(hipMalloc((void**)&d_thin, (size_t)n * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_thin_colours, (size_t)n * 3));
    HIP_OK(hipMalloc((void**)&d_counts, (size_t)n * sizeof(int)));
    HIP_OK(hipMalloc(&d_thin_work, (size_t)thin_bytes));
    CHECK(snerf_voxel_thin(d_in, d_in_colours, n, 0.0, lo[0], lo[1], lo[2], extents[0], extents[1], extents[2], d_thin, d_thin_colours,
                           d_counts, d_count + 1, d_thin_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_voxel_thin(d_in, d_in_colours, n, voxel_size, lo[0], (double)INFINITY, lo[2], extents[0], extents[1], extents[2], d_thin,
                           d_thin_colours, d_counts, d_count + 1, d_thin_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_voxel_thin(d_in, d_in_colours, n, voxel_size, lo[0], lo[1], lo[2], 65536, 65536, 1, d_thin, d_thin_colours, d_counts,
                           d_count + 1, d_thin_work, nullptr) == SNERF_E_UNSUPPORTED);
    SNERF_OK_(snerf_voxel_thin(d_in, d_in_colours, n, voxel_size, lo[0], lo[1], lo[2], extents[0], extents[1], extents[2], d_thin,
                               d_thin_colours, d_counts, d_count + 1, d_thin_work, nullptr));
    HIP_OK(hipDeviceSynchronize());
    long long got_m = -1;
    HIP_OK(hipMemcpy(&got_m, d_count + 1, sizeof(long long), hipMemcpyDeviceToHost));
    std::printf("fuse_abi_smoke: thinned to %lld voxels, expected %lld\n", got_m, m);
    CHECK(got_m == m);
    std::vector<float> thin((size_t)m * 3);
    std::vector<unsigned char> thin_colours((size_t)m * 3);
    std::vector<int32_t> counts((size_t)m);
    HIP_OK(hipMemcpy(thin.data(), d_thin, thin.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(thin_colours.data(), d_thin_colours, thin_colours.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(counts.data(), d_counts, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (long long record : {0LL, m - 1}) {
        CHECK(std::memcmp(&thin[3 * record], &want_thin[3 * record], 3 * sizeof(float)) == 0);
        CHECK(std::memcmp(&thin_colours[3 * record], &want_thin_colours[3 * record], 3) == 0);
        CHECK(counts[record] == want_counts[record]);
    }
    for (void* p : {(void*)d_cameras, (void*)d_depth, (void*)d_image, (void*)d_points, (void*)d_colours, (void*)d_views, (void*)d_count, d_work,
                    (void*)d_in, (void*)d_in_colours, (void*)d_thin, (void*)d_thin_colours, (void*)d_counts, d_thin_work})
        HIP_OK(hipFree(p));
    std::printf("fuse_abi_smoke: OK\n");
    return 0;
}
