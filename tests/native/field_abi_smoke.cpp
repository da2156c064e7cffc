// The density mesh from the C ABI alone: plain HIP runtime + include/simplenerf_hip.h + csrc/simplenerf_field.h, linked against
// libsimplenerf_hip.so, no PyTorch in the process.
//
//   field_abi_smoke <fixture file>
//
// The fixture (tests/field_reference.py: native_fixture) holds the analytic scene's cameras, a grid over it with the restated points
// and weights of its nodes, and a small seeded MLP.  snerf_field_grid_points must give the fixture's weights and points (equal or
// adjacent floats), as a whole and in two blocks; snerf_mlp_pack_for + snerf_mlp_forward give the densities at those points,
// snerf_field_values the volume of the fixture's level, snerf_mesh_count / snerf_mesh_emit its mesh, whose counts are printed (and
// compared when the fixture knows them); snerf_field_point_views runs on the mesh's vertices; the refusals are status codes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simplenerf_hip.h"
#include "simplenerf_field.h"

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
    if (argc != 2) return std::printf("usage: field_abi_smoke fixture\n"), 1;
    CHECK(snerf_abi_version() == SNERF_ABI_VERSION);
    Reader in;
    CHECK(read_file(argv[1], in.bytes));
    const int views = in.one<int32_t>(), h = in.one<int32_t>(), w = in.one<int32_t>();
    const int nx = in.one<int32_t>(), ny = in.one<int32_t>(), nz = in.one<int32_t>(), np = in.one<int32_t>();
    const double voxel = in.one<double>();
    double lo[3];
    for (double& v : lo) v = in.one<double>();
    const double level = in.one<double>();
    const long long want_nv = in.one<int64_t>(), want_nt = in.one<int64_t>();
    CHECK(in.ok && views >= 1 && views <= SNERF_FUSE_MAX_VIEWS && h >= 1 && w >= 1 && h <= 4096 && w <= 4096);
    CHECK(nx >= 2 && ny >= 2 && nz >= 2 && nx <= 512 && ny <= 512 && nz <= 512 && level > 0.0);
    const long long nodes = (long long)nx * ny * nz;
    const std::vector<double> cameras = in.many<double>((size_t)views * SNERF_FUSE_CAMERA_DOUBLES);
    const std::vector<float> want_points = in.many<float>((size_t)nodes * 3);
    const std::vector<unsigned char> want_weight = in.many<unsigned char>((size_t)nodes);
    snerf_mlp_desc desc = {4, 128, 1, 64, 10, 4, -1, 1, 1};
    CHECK(in.ok && np == snerf_mlp_num_params(&desc) && np == 16);
    std::vector<float*> params(np, nullptr);
    for (int i = 0; i < np; ++i) {
        const long long count = in.one<int64_t>();
        CHECK(in.ok && count >= 1 && count <= (1 << 20));
        const std::vector<float> values = in.many<float>((size_t)count);
        CHECK(in.ok);
        HIP_OK(upload(values, &params[i]));
    }
    CHECK(in.at == in.bytes.size());

    double* d_cameras = nullptr;
    float* d_points = nullptr;
    unsigned char* d_weight = nullptr;
    HIP_OK(upload(cameras, &d_cameras));
    HIP_OK(hipMalloc((void**)&d_points, (size_t)(nodes + 1) * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_weight, (size_t)nodes + 1));
    HIP_OK(hipMemset(d_points, 0xAA, (size_t)(nodes + 1) * 3 * sizeof(float)));
    HIP_OK(hipMemset(d_weight, 0xAA, (size_t)nodes + 1));

    // ---- the grid's points; every refusal comes before the first launch
    auto grid_points = [&](double size, int ex, long long first, long long count, int v, int ndc, double near_plane, float* out_points,
                           const double* table) {
        return snerf_field_grid_points(size, lo[0], lo[1], lo[2], ex, ny, nz, first, count, table, v, h, w, ndc, -1.5, -2.0, near_plane,
                                       out_points, d_weight, nullptr);
    };
    CHECK(grid_points(0.0, nx, 0, nodes, views, 0, 1.0, d_points, d_cameras) == SNERF_E_INVALID);
    CHECK(grid_points(voxel, 0, 0, nodes, views, 0, 1.0, d_points, d_cameras) == SNERF_E_INVALID);
    CHECK(grid_points(voxel, nx, -1, 1, views, 0, 1.0, d_points, d_cameras) == SNERF_E_INVALID);
    CHECK(grid_points(voxel, nx, 1, nodes, views, 0, 1.0, d_points, d_cameras) == SNERF_E_INVALID);
    CHECK(grid_points(voxel, nx, 0, -1, views, 0, 1.0, d_points, d_cameras) == SNERF_E_INVALID);
    CHECK(grid_points(voxel, nx, 0, nodes, SNERF_FUSE_MAX_VIEWS + 1, 0, 1.0, d_points, d_cameras) == SNERF_E_INVALID);
    CHECK(grid_points(voxel, nx, 0, nodes, views, 1, 0.0, d_points, d_cameras) == SNERF_E_INVALID);
    CHECK(grid_points(voxel, nx, 0, nodes, views, 1, (double)NAN, d_points, d_cameras) == SNERF_E_INVALID);
    CHECK(grid_points(voxel, nx, 0, nodes, views, 0, 1.0, nullptr, d_cameras) == SNERF_E_INVALID);
    CHECK(grid_points(voxel, nx, 0, nodes, views, 0, 1.0, d_points, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_field_grid_points(voxel, lo[0], lo[1], lo[2], 1024, 1024, 1024, 0, 1, d_cameras, views, h, w, 0, 0.0, 0.0, 0.0, d_points, d_weight,
                                  nullptr) == SNERF_E_UNSUPPORTED);
    CHECK(grid_points(voxel, nx, nodes, 0, views, 0, 1.0, nullptr, nullptr) == SNERF_OK);     // (nothing to do: nothing enqueued)
    SNERF_OK_(grid_points(voxel, nx, 0, nodes, views, 0, 0.0, d_points, d_cameras));
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> points((size_t)(nodes + 1) * 3);
    std::vector<unsigned char> weight((size_t)nodes + 1);
    HIP_OK(hipMemcpy(points.data(), d_points, points.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(weight.data(), d_weight, weight.size(), hipMemcpyDeviceToHost));
    long long seen = 0;
    for (long long n = 0; n < nodes; ++n) {
        CHECK(weight[n] == want_weight[n]);
        for (int a = 0; a < 3; ++a) CHECK(adjacent(points[3 * n + a], want_points[3 * n + a]));
        seen += weight[n] > 0;
    }
    uint32_t bits;     // rows past the count are not written
    std::memcpy(&bits, &points[3 * nodes], 4);
    CHECK(bits == 0xAAAAAAAAu && weight[nodes] == 0xAA);
    // two blocks give the rows of the whole
    const long long split = nodes / 3;
    float* d_blocks = nullptr;
    unsigned char* d_whole_weight = d_weight;
    HIP_OK(hipMalloc((void**)&d_blocks, (size_t)nodes * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_weight, (size_t)nodes));
    SNERF_OK_(snerf_field_grid_points(voxel, lo[0], lo[1], lo[2], nx, ny, nz, 0, split, d_cameras, views, h, w, 0, 0.0, 0.0, 0.0, d_blocks,
                                      d_weight, nullptr));
    SNERF_OK_(snerf_field_grid_points(voxel, lo[0], lo[1], lo[2], nx, ny, nz, split, nodes - split, d_cameras, views, h, w, 0, 0.0, 0.0, 0.0,
                                      d_blocks + 3 * split, d_weight + split, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> block_points((size_t)nodes * 3);
    std::vector<unsigned char> block_weight((size_t)nodes);
    HIP_OK(hipMemcpy(block_points.data(), d_blocks, block_points.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(block_weight.data(), d_weight, block_weight.size(), hipMemcpyDeviceToHost));
    CHECK(std::memcmp(block_points.data(), points.data(), block_points.size() * sizeof(float)) == 0);
    CHECK(std::memcmp(block_weight.data(), weight.data(), block_weight.size()) == 0);
    std::printf("field_abi_smoke: %lld nodes, %lld seen\n", nodes, seen);

    // ---- the field at the nodes: every node a ray of one sample at depth 0
    float *d_packed = nullptr, *d_zero = nullptr, *d_dirs = nullptr, *d_sigma = nullptr, *d_rgb = nullptr, *d_tsdf = nullptr;
    HIP_OK(hipMalloc((void**)&d_packed, snerf_mlp_packed_floats(&desc) * sizeof(float)));
    HIP_OK(hipMemset(d_packed, 0, snerf_mlp_packed_floats(&desc) * sizeof(float)));
    SNERF_OK_(snerf_mlp_pack_for(&desc, params.data(), np, d_packed, SNERF_PRECISION_FP32, 0, nullptr));
    std::vector<float> down((size_t)nodes * 3, 0.f);
    for (long long n = 0; n < nodes; ++n) down[3 * n + 2] = -1.f;
    HIP_OK(upload(down, &d_dirs));
    HIP_OK(hipMalloc((void**)&d_zero, (size_t)nodes * 3 * sizeof(float)));
    HIP_OK(hipMemset(d_zero, 0, (size_t)nodes * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_sigma, (size_t)nodes * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_rgb, (size_t)nodes * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_tsdf, (size_t)nodes * sizeof(float)));
    SNERF_OK_(snerf_mlp_forward(&desc, d_packed, d_blocks, d_zero, d_dirs, d_zero, nodes, 1, nullptr, d_sigma, d_rgb, SNERF_PRECISION_FP32,
                                nullptr));
    CHECK(snerf_field_values(d_sigma, d_weight, nodes, 0.0, d_tsdf, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_field_values(d_sigma, d_weight, nodes, (double)INFINITY, d_tsdf, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_field_values(d_sigma, d_weight, -1, level, d_tsdf, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_field_values(d_sigma, nullptr, nodes, level, d_tsdf, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_field_values(d_sigma, d_weight, 1LL << 31, level, d_tsdf, nullptr) == SNERF_E_UNSUPPORTED);
    CHECK(snerf_field_values(nullptr, nullptr, 0, level, nullptr, nullptr) == SNERF_OK);
    SNERF_OK_(snerf_field_values(d_sigma, d_weight, nodes, level, d_tsdf, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> sigma((size_t)nodes), tsdf((size_t)nodes);
    HIP_OK(hipMemcpy(sigma.data(), d_sigma, sigma.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(tsdf.data(), d_tsdf, tsdf.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (long long n = 0; n < nodes; ++n) {
        CHECK(sigma[n] >= 0.f);
        const double t = std::fmin(1.0, std::fmax(-1.0, (level - (double)sigma[n]) / level));
        CHECK(tsdf[n] == (weight[n] == 0 ? 1.0f : (float)t));
    }

    // ---- the mesh of that volume
    const long long bytes = snerf_mesh_workspace_bytes(nx, ny, nz);
    CHECK(bytes > 0);
    long long* d_counts = nullptr;
    void* d_work = nullptr;
    HIP_OK(hipMalloc((void**)&d_counts, 2 * sizeof(long long)));
    HIP_OK(hipMalloc(&d_work, (size_t)bytes));
    SNERF_OK_(snerf_mesh_count(d_tsdf, d_weight, voxel, lo[0], lo[1], lo[2], nx, ny, nz, 1, d_counts, d_work, nullptr));
    HIP_OK(hipDeviceSynchronize());
    long long counts[2] = {-1, -1};
    HIP_OK(hipMemcpy(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost));
    std::printf("field_abi_smoke: %lld nodes, %lld vertices, %lld triangles\n", nodes, counts[0], counts[1]);
    CHECK(counts[0] >= 0 && counts[1] >= 0 && counts[0] <= SNERF_MESH_KEYS_PER_NODE * nodes && counts[1] <= 12 * nodes);
    CHECK((want_nv < 0 || counts[0] == want_nv) && (want_nt < 0 || counts[1] == want_nt));
    float *d_vertices = nullptr, *d_mlp_points = nullptr, *d_view_dirs = nullptr;
    int* d_triangles = nullptr;
    unsigned char* d_view = nullptr;
    const size_t nv = (size_t)counts[0], nt = (size_t)counts[1];
    HIP_OK(hipMalloc((void**)&d_vertices, (nv + 1) * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_triangles, (nt + 1) * 3 * sizeof(int)));
    HIP_OK(hipMalloc((void**)&d_mlp_points, (nv + 1) * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_view_dirs, (nv + 1) * 3 * sizeof(float)));
    HIP_OK(hipMalloc((void**)&d_view, nv + 1));
    if (nv > 0 && nt > 0)
        SNERF_OK_(snerf_mesh_emit(d_tsdf, d_weight, voxel, lo[0], lo[1], lo[2], nx, ny, nz, 1, d_counts, d_vertices, d_triangles, d_work, nullptr));

    // ---- a view for every vertex
    CHECK(snerf_field_point_views(d_vertices, (long long)nv, d_cameras, 0, h, w, 0, 0.0, 0.0, 0.0, d_mlp_points, d_view_dirs, d_view, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_field_point_views(d_vertices, -1, d_cameras, views, h, w, 0, 0.0, 0.0, 0.0, d_mlp_points, d_view_dirs, d_view, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_field_point_views(d_vertices, 1, d_cameras, views, h, w, 1, 1.0, 1.0, -1.0, d_mlp_points, d_view_dirs, d_view, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_field_point_views(d_vertices, 1, d_cameras, views, h, w, 0, 0.0, 0.0, 0.0, d_mlp_points, nullptr, d_view, nullptr) ==
          SNERF_E_INVALID);
    CHECK(snerf_field_point_views(d_vertices, 1LL << 31, d_cameras, views, h, w, 0, 0.0, 0.0, 0.0, d_mlp_points, d_view_dirs, d_view, nullptr) ==
          SNERF_E_UNSUPPORTED);
    CHECK(snerf_field_point_views(nullptr, 0, nullptr, views, h, w, 0, 0.0, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr) == SNERF_OK);
    SNERF_OK_(snerf_field_point_views(d_vertices, (long long)nv, d_cameras, views, h, w, 0, 0.0, 0.0, 0.0, d_mlp_points, d_view_dirs, d_view,
                                      nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<float> vertices(nv * 3), mlp_points(nv * 3), view_dirs(nv * 3);
    std::vector<unsigned char> view(nv);
    HIP_OK(hipMemcpy(vertices.data(), d_vertices, vertices.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(mlp_points.data(), d_mlp_points, mlp_points.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(view_dirs.data(), d_view_dirs, view_dirs.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(view.data(), d_view, view.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nv; ++i) {
        CHECK(view[i] < views || view[i] == SNERF_FIELD_NO_VIEW);
        double norm = 0.0;
        for (int a = 0; a < 3; ++a) {
            CHECK(mlp_points[3 * i + a] == vertices[3 * i + a]);      // (without ndc the MLP reads the point itself)
            norm += (double)view_dirs[3 * i + a] * view_dirs[3 * i + a];
        }
        CHECK(std::fabs(norm - 1.0) < 1e-6);
    }
    for (float* p : params) HIP_OK(hipFree(p));
    for (void* p : {(void*)d_cameras, (void*)d_points, (void*)d_whole_weight, (void*)d_blocks, (void*)d_weight, (void*)d_packed, (void*)d_zero,
                    (void*)d_dirs, (void*)d_sigma, (void*)d_rgb, (void*)d_tsdf, (void*)d_counts, d_work, (void*)d_vertices, (void*)d_triangles,
                    (void*)d_mlp_points, (void*)d_view_dirs, (void*)d_view})
        HIP_OK(hipFree(p));
    std::printf("field_abi_smoke: OK\n");
    return 0;
}
