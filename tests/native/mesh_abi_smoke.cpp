// The mesh export from the C ABI alone: plain HIP runtime + include/simplenerf_hip.h + csrc/simplenerf_mesh.h, linked against
// libsimplenerf_hip.so, no PyTorch in the process.
//
//   mesh_abi_smoke <fixture file>
//
// The fixture (tests/mesh_reference.py: native_fixture) holds the analytic scene, the restated volume of it, the restated mesh of
// that volume and the restated colours of those vertices.  snerf_tsdf_integrate must give the fixture's weights and its distances
// (equal or adjacent floats); snerf_mesh_count / snerf_mesh_emit on the fixture's volume must give its two counts and its first and
// last vertex (equal or adjacent floats) and triangle; snerf_colour_points on the fixture's vertices its first and last colour and
// view count; the refusals are status codes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simplenerf_hip.h"
#include "simplenerf_mesh.h"

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
    if (argc != 2) return std::printf("usage: mesh_abi_smoke fixture\n"), 1;
    CHECK(snerf_abi_version() == SNERF_ABI_VERSION);
    Reader in;
    CHECK(read_file(argv[1], in.bytes));
    const int views = in.one<int32_t>(), h = in.one<int32_t>(), w = in.one<int32_t>();
    const int nx = in.one<int32_t>(), ny = in.one<int32_t>(), nz = in.one<int32_t>(), min_weight = in.one<int32_t>();
    const double voxel = in.one<double>();
    double lo[3];
    for (double& v : lo) v = in.one<double>();
    const double mu = in.one<double>(), tolerance = in.one<double>();
    CHECK(in.ok && views >= 1 && views <= SNERF_FUSE_MAX_VIEWS && h >= 1 && w >= 1 && h <= 4096 && w <= 4096);
    CHECK(nx >= 2 && ny >= 2 && nz >= 2 && nx <= 512 && ny <= 512 && nz <= 512);
    const size_t total = (size_t)views * h * w, nodes = (size_t)nx * ny * nz;
    const std::vector<double> cameras = in.many<double>((size_t)views * SNERF_FUSE_CAMERA_DOUBLES);
    const std::vector<float> depth = in.many<float>(total);
    const std::vector<unsigned char> image = in.many<unsigned char>(total * 3);
    const std::vector<float> want_tsdf = in.many<float>(nodes);
    const std::vector<unsigned char> want_weight = in.many<unsigned char>(nodes);
    const long long nv = in.one<int64_t>(), nt = in.one<int64_t>();
    CHECK(in.ok && nv >= 1 && nt >= 1 && (size_t)nv <= SNERF_MESH_KEYS_PER_NODE * nodes && (size_t)nt <= 12 * nodes);
    const std::vector<float> want_vertices = in.many<float>((size_t)nv * 3);
    const std::vector<int32_t> want_triangles = in.many<int32_t>((size_t)nt * 3);
    const std::vector<unsigned char> want_colours = in.many<unsigned char>((size_t)nv * 3);
    const std::vector<unsigned char> want_views = in.many<unsigned char>((size_t)nv);
    CHECK(in.ok && in.at == in.bytes.size());

    double* d_cameras = nullptr;
    float *d_depth = nullptr, *d_tsdf = nullptr;
    unsigned char *d_image = nullptr, *d_weight = nullptr;
    HIP_OK(upload(cameras, &d_cameras));
    HIP_OK(upload(depth, &d_depth));
    HIP_OK(upload(image, &d_image));
    HIP_OK(hipMalloc((void**)&d_tsdf, nodes * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_weight, nodes));

    // ---- the integration; every refusal comes before the first launch
    CHECK(snerf_tsdf_integrate(d_depth, nullptr, d_cameras, views, h, w, 0.0, lo[0], lo[1], lo[2], nx, ny, nz, mu, d_tsdf, d_weight, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_tsdf_integrate(d_depth, nullptr, d_cameras, views, h, w, voxel, lo[0], lo[1], lo[2], nx, ny, nz, 0.0, d_tsdf, d_weight, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_tsdf_integrate(d_depth, nullptr, d_cameras, views, h, w, voxel, lo[0], (double)NAN, lo[2], nx, ny, nz, mu, d_tsdf, d_weight,
                               nullptr) == SNERF_E_INVALID);
    CHECK(snerf_tsdf_integrate(d_depth, nullptr, d_cameras, views, h, w, voxel, lo[0], lo[1], lo[2], nx, 0, nz, mu, d_tsdf, d_weight, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_tsdf_integrate(nullptr, nullptr, d_cameras, views, h, w, voxel, lo[0], lo[1], lo[2], nx, ny, nz, mu, d_tsdf, d_weight, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_tsdf_integrate(d_depth, nullptr, d_cameras, SNERF_FUSE_MAX_VIEWS + 1, h, w, voxel, lo[0], lo[1], lo[2], nx, ny, nz, mu, d_tsdf,
                               d_weight, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_tsdf_integrate(d_depth, nullptr, d_cameras, views, h, w, voxel, lo[0], lo[1], lo[2], 1024, 1024, 1024, mu, d_tsdf, d_weight,
                               nullptr) == SNERF_E_UNSUPPORTED);
    SNERF_OK_(snerf_tsdf_integrate(d_depth, nullptr, d_cameras, views, h, w, voxel, lo[0], lo[1], lo[2], nx, ny, nz, mu, d_tsdf, d_weight, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> tsdf(nodes);
    std::vector<unsigned char> weight(nodes);
    HIP_OK(hipMemcpy(tsdf.data(), d_tsdf, nodes * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(weight.data(), d_weight, nodes, hipMemcpyDeviceToHost));
    size_t observed = 0;
    for (size_t n = 0; n < nodes; ++n) {
        CHECK(weight[n] == want_weight[n]);
        CHECK(adjacent(tsdf[n], want_tsdf[n]) && (tsdf[n] < 0.0f) == (want_tsdf[n] < 0.0f));
        observed += weight[n] > 0;
    }
    std::printf("mesh_abi_smoke: integrated %zu nodes, %zu observed\n", nodes, observed);

    // ---- the extraction, of the fixture's own volume
    const long long bytes = snerf_mesh_workspace_bytes(nx, ny, nz);
    CHECK(bytes >= (long long)(10 * nodes));
    CHECK(snerf_mesh_workspace_bytes(0, ny, nz) == 0 && snerf_mesh_workspace_bytes(1024, 1024, 1024) == 0 &&
          snerf_mesh_workspace_bytes(1, 1, 1) > 0);
    long long* d_counts = nullptr;
    void* d_work = nullptr;
    float* d_vertices = nullptr;
    int* d_triangles = nullptr;
    HIP_OK(hipMemcpy(d_tsdf, want_tsdf.data(), nodes * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_weight, want_weight.data(), nodes, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc((void**)&d_counts, 2 * sizeof(long long)));
    HIP_OK(hipMalloc(&d_work, (size_t)bytes));
    CHECK(snerf_mesh_count(d_tsdf, d_weight, voxel, lo[0], lo[1], lo[2], nx, ny, nz, 0, d_counts, d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_mesh_count(d_tsdf, d_weight, voxel, lo[0], lo[1], lo[2], nx, ny, nz, 256, d_counts, d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_mesh_count(d_tsdf, nullptr, voxel, lo[0], lo[1], lo[2], nx, ny, nz, min_weight, d_counts, d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_mesh_count(d_tsdf, d_weight, voxel, lo[0], lo[1], lo[2], nx, ny, nz, min_weight, d_counts, (char*)d_work + 8, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_mesh_count(d_tsdf, d_weight, -1.0, lo[0], lo[1], lo[2], nx, ny, nz, min_weight, d_counts, d_work, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_mesh_count(d_tsdf, d_weight, voxel, lo[0], lo[1], lo[2], 1024, 1024, 1024, min_weight, d_counts, d_work, nullptr) ==
          SNERF_E_UNSUPPORTED);
    SNERF_OK_(snerf_mesh_count(d_tsdf, d_weight, voxel, lo[0], lo[1], lo[2], nx, ny, nz, min_weight, d_counts, d_work, nullptr));
    HIP_OK(hipDeviceSynchronize());
    long long counts[2] = {-1, -1};
    HIP_OK(hipMemcpy(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost));
    std::printf("mesh_abi_smoke: counted %lld vertices and %lld triangles, expected %lld and %lld\n", counts[0], counts[1], nv, nt);
    CHECK(counts[0] == nv && counts[1] == nt);
    HIP_OK(hipMalloc((void**)&d_vertices, ((size_t)nv + 1) * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_triangles, ((size_t)nt + 1) * 3 * sizeof(int)));
    HIP_OK(hipMemset(d_vertices, 0xAA, ((size_t)nv + 1) * 3 * sizeof(float)));
    HIP_OK(hipMemset(d_triangles, 0xAA, ((size_t)nt + 1) * 3 * sizeof(int)));
    CHECK(snerf_mesh_emit(d_tsdf, d_weight, voxel, lo[0], lo[1], lo[2], nx, ny, nz, min_weight, d_counts, nullptr, d_triangles, d_work, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_mesh_emit(d_tsdf, d_weight, voxel, lo[0], lo[1], lo[2], nx, ny, nz, min_weight, nullptr, d_vertices, d_triangles, d_work, nullptr) ==
          SNERF_E_INVALID);
    SNERF_OK_(snerf_mesh_emit(d_tsdf, d_weight, voxel, lo[0], lo[1], lo[2], nx, ny, nz, min_weight, d_counts, d_vertices, d_triangles, d_work,
                              nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> vertices(((size_t)nv + 1) * 3);
    std::vector<int32_t> triangles(((size_t)nt + 1) * 3);
    HIP_OK(hipMemcpy(vertices.data(), d_vertices, vertices.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(triangles.data(), d_triangles, triangles.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (long long record : {0LL, nv - 1})
        for (int a = 0; a < 3; ++a) CHECK(adjacent(vertices[3 * record + a], want_vertices[3 * record + a]));
    for (long long record : {0LL, nt - 1})
        for (int a = 0; a < 3; ++a) CHECK(triangles[3 * record + a] == want_triangles[3 * record + a]);
    for (long long i = 0; i < 3 * nt; ++i) CHECK(triangles[i] >= 0 && triangles[i] < nv);
    uint32_t bits;     // rows past the counts are not written
    std::memcpy(&bits, &vertices[3 * nv], 4);
    CHECK(bits == 0xAAAAAAAAu);
    std::memcpy(&bits, &triangles[3 * nt], 4);
    CHECK(bits == 0xAAAAAAAAu);

    // ---- the colours, of the fixture's own vertices
    float* d_points = nullptr;
    unsigned char *d_colours = nullptr, *d_agreeing = nullptr;
    HIP_OK(upload(want_vertices, &d_points));
    HIP_OK(hipMalloc((void**)&d_colours, (size_t)nv * 3));
    HIP_OK(hipMalloc((void**)&d_agreeing, (size_t)nv));
    CHECK(snerf_colour_points(d_points, nv, d_depth, d_image, nullptr, d_cameras, views, h, w, -1.0, d_colours, d_agreeing, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_colour_points(d_points, -1, d_depth, d_image, nullptr, d_cameras, views, h, w, tolerance, d_colours, d_agreeing, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_colour_points(d_points, nv, d_depth, nullptr, nullptr, d_cameras, views, h, w, tolerance, d_colours, d_agreeing, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_colour_points(nullptr, nv, d_depth, d_image, nullptr, d_cameras, views, h, w, tolerance, d_colours, d_agreeing, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_colour_points(nullptr, 0, nullptr, nullptr, nullptr, nullptr, views, h, w, tolerance, nullptr, nullptr, nullptr) ==
          SNERF_OK);     // (nothing to do: nothing enqueued)
    SNERF_OK_(snerf_colour_points(d_points, nv, d_depth, d_image, nullptr, d_cameras, views, h, w, tolerance, d_colours, d_agreeing, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<unsigned char> colours((size_t)nv * 3), agreeing((size_t)nv);
    HIP_OK(hipMemcpy(colours.data(), d_colours, colours.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(agreeing.data(), d_agreeing, agreeing.size(), hipMemcpyDeviceToHost));
    for (long long record : {0LL, nv - 1}) {
        CHECK(std::memcmp(&colours[3 * record], &want_colours[3 * record], 3) == 0);
        CHECK(agreeing[record] == want_views[record]);
    }
    std::printf("mesh_abi_smoke: coloured %lld vertices\n", nv);
    for (void* p : {(void*)d_cameras, (void*)d_depth, (void*)d_image, (void*)d_tsdf, (void*)d_weight, (void*)d_counts, d_work, (void*)d_vertices,
                    (void*)d_triangles, (void*)d_points, (void*)d_colours, (void*)d_agreeing})
        HIP_OK(hipFree(p));
    std::printf("mesh_abi_smoke: OK\n");
    return 0;
}
