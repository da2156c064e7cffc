// The surface export (simplenerf_mesh.h): depth maps on the device -> a truncated signed distance volume -> a triangle mesh by
// marching tetrahedra, and colours for its vertices from the frames.
//
// snerf_tsdf_integrate, one launch: a thread per node (x fastest: neighbouring nodes land on neighbouring pixels, the camera rows
//   are uniform over a wave) looks its node up in every view in ascending order and averages the truncated distances.
// snerf_mesh_count, five launches:
//   cells    a thread per node as a cell origin: one byte, 0 for no or an incomplete cell, else 0x80 | its number of triangles
//   edges    a workgroup per tile of 2048 nodes (sort_plan.h's tiling): a thread decides the seven edges that start at its nodes --
//            signs differ, a complete cell contains it -- by reading (nobody marks an edge), stores them as one mask byte per node
//            and adds up the tile's vertices and triangles (both in one uint32: a tile has at most 14336 and 24576)
//   scan x 2 the tile counters, exclusively
//   firsts   a workgroup per tile: wave scans in (wave, round, lane) = index order give every node the number of its first vertex
//            and of its cell's first triangle; the last tile writes the two totals
// snerf_mesh_emit, one launch: a thread per node writes its node's vertices and its cell's triangles at those numbers; the number
//   of a referenced vertex is its node's first plus the set mask bits below its type.
// snerf_colour_points, one launch: a thread per point.
// No atomics, one owner per output element, fp64 throughout (the library is built with -ffp-contract=off).
// Bound: the integration and the colouring by the fp64 divide rate and the dependent depth reads per view; the extraction by memory
// latency (8 to 27 neighbouring bytes and floats a node, all from cache lines its neighbours share).
#include <cfloat>
#include <cmath>

#include "snerf_common.h"
#include "simplenerf_mesh.h"
#include "mesh_lookup.h"
#include "mesh_tables.h"
#include "sort_plan.h"
#include "tile_scan.h"

namespace {

using namespace snerf::sortplan;
using namespace snerf::tilescan;
using namespace snerf::mesh;

static_assert(kKeysPerNode == SNERF_MESH_KEYS_PER_NODE, "mesh_tables.h and simplenerf_mesh.h number the same keys");
constexpr unsigned char kComplete = 0x80;                      // cell byte: kComplete | triangles (0 .. 12)

struct Views {
    const float* depth;
    const unsigned char* mask;      // or NULL
    const double* cameras;
    int views, height, width;
    long long pixels;               // height * width
};

// The lookup of P in view u: false when the view does not see P or the pixel it lands on is not valid; else *c_z is P's depth in
// the view and *pixel the index of that pixel in (views, height, width).
__device__ __forceinline__ bool look_up(const Views& f, const double P[3], int u, double* c_z, long long* pixel) {
    double ix, iy;
    if (!view_pixel(f.cameras, u, f.height, f.width, P, c_z, &ix, &iy)) return false;
    const long long j = (long long)u * f.pixels + (long long)iy * f.width + (long long)ix;
    const float d = f.depth[j];
    if (!(d > 0.0f && d <= FLT_MAX) || (f.mask && f.mask[j] == 0)) return false;
    *pixel = j;
    return true;
}

// the node index of n's neighbour at offset code `code` (bit 0 = x, bit 1 = y, bit 2 = z)
__device__ __forceinline__ long long neighbour(const Grid& g, long long n, int code) {
    return n + (code & 1) + (long long)((code >> 1) & 1) * g.n[0] + (long long)((code >> 2) & 1) * g.n[0] * g.n[1];
}

// ------------------------------------------------------------------------------------------------ integrate
// grid (ceil(nodes / kBlock))
__global__ void __launch_bounds__(kBlock) tsdf_integrate_kernel(Views f, Grid g, double mu, float* __restrict__ tsdf,
                                                                unsigned char* __restrict__ weight) {
    const long long n = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (n >= g.nodes) return;
    int at[3];
    node_index(g, n, at);
    double P[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) P[a] = g.lo[a] + g.voxel_size * (double)at[a];
    double sum = 0.0;
    int count = 0;
    for (int u = 0; u < f.views; ++u) {
        double c_z;
        long long pixel;
        if (!look_up(f, P, u, &c_z, &pixel)) continue;
        const double s = (double)f.depth[pixel] - c_z;
        if (!(s >= -mu)) continue;
        sum += fmin(1.0, s / mu);
        ++count;
    }
    tsdf[n] = count > 0 ? (float)(sum / (double)count) : 1.0f;
    weight[n] = (unsigned char)count;
}

// ------------------------------------------------------------------------------------------------ colour
// grid (ceil(count / kBlock))
__global__ void __launch_bounds__(kBlock) colour_points_kernel(const float* __restrict__ points, long long count, Views f,
                                                               const unsigned char* __restrict__ image, double tolerance,
                                                               unsigned char* __restrict__ colours, unsigned char* __restrict__ agreeing) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const double P[3] = {(double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2]};
    unsigned sum[3] = {0u, 0u, 0u}, n = 0;
    for (int u = 0; u < f.views; ++u) {
        double c_z;
        long long pixel;
        if (!look_up(f, P, u, &c_z, &pixel)) continue;
        if (!(fabs(c_z - (double)f.depth[pixel]) <= tolerance)) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) sum[a] += image[3 * pixel + a];
        ++n;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) colours[3 * i + a] = n ? (unsigned char)((2u * sum[a] + n) / (2u * n)) : (unsigned char)0;
    agreeing[i] = (unsigned char)n;
}

// ------------------------------------------------------------------------------------------------ extract
// bit `code` of the result: the node at offset `code` of cell n is negative.  The cell must exist (n's indices below n_a - 1).
__device__ __forceinline__ unsigned cell_signs(const float* __restrict__ tsdf, const Grid& g, long long n) {
    unsigned signs = 0;
#pragma unroll
    for (int code = 0; code < 8; ++code) signs |= (tsdf[neighbour(g, n, code)] < 0.0f ? 1u : 0u) << code;
    return signs;
}

__device__ __forceinline__ int tetrahedron_case(unsigned signs, int t) {
    int c = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) c |= (int)((signs >> kTetVertex[t][m]) & 1u) << m;
    return c;
}

// grid (ceil(nodes / kBlock)): cell[n] of every node as a cell origin
__global__ void __launch_bounds__(kBlock) mesh_cells_kernel(const float* __restrict__ tsdf, const unsigned char* __restrict__ weight,
                                                            Grid g, int min_weight, unsigned char* __restrict__ cell) {
    const long long n = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (n >= g.nodes) return;
    int at[3];
    node_index(g, n, at);
    unsigned char out = 0;
    if (at[0] < g.n[0] - 1 && at[1] < g.n[1] - 1 && at[2] < g.n[2] - 1) {
        bool complete = true;
#pragma unroll
        for (int code = 0; code < 8; ++code) complete = complete && (int)weight[neighbour(g, n, code)] >= min_weight;
        if (complete) {
            const unsigned signs = cell_signs(tsdf, g, n);
            int triangles = 0;
#pragma unroll
            for (int t = 0; t < kTetrahedra; ++t) triangles += kTetCase[t][tetrahedron_case(signs, t)].triangles;
            out = (unsigned char)(kComplete | triangles);
        }
    }
    cell[n] = out;
}

// Bit `type` of the result: the edge of that type from node n < nodes is a mesh vertex.
__device__ __forceinline__ unsigned edge_mask(const float* __restrict__ tsdf, const unsigned char* __restrict__ cell, const Grid& g,
                                              long long n) {
    int at[3];
    node_index(g, n, at);
    const bool negative = tsdf[n] < 0.0f;
    unsigned mask = 0;
#pragma unroll
    for (int type = 0; type < kKeysPerNode; ++type) {
        const int code = kOffsetOfType[type];
        bool inside = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) inside = inside && at[a] + ((code >> a) & 1) < g.n[a];
        if (!inside || (tsdf[neighbour(g, n, code)] < 0.0f) == negative) continue;
        // the cells that contain it: along an axis the edge spans, the origin is A's index; along the others, that or one below
        bool found = false;
        for (int back = 0; back < 8 && !found; ++back) {
            if (back & code) continue;
            long long origin = n;
            bool exists = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int o = at[a] - ((back >> a) & 1);
                exists = exists && o >= 0 && o < g.n[a] - 1;
            }
            if (!exists) continue;
            origin -= (back & 1) + (long long)((back >> 1) & 1) * g.n[0] + (long long)((back >> 2) & 1) * g.n[0] * g.n[1];
            found = (cell[origin] & kComplete) != 0;
        }
        if (found) mask |= 1u << type;
    }
    return mask;
}

// vertices of a node in the low half, triangles of its cell in the high half (a wave's 512 nodes: 3584 and 6144 at the most)
__device__ __forceinline__ uint32_t packed_counts(unsigned char vertex_mask, unsigned char cell_byte) {
    return (uint32_t)__popc((unsigned)vertex_mask) | ((uint32_t)(cell_byte & 0x7F) << 16);
}

// grid (tiles): vertex_mask[n] of every node of the tile; the tile's vertices and triangles
__global__ void __launch_bounds__(kBlock) mesh_edges_kernel(const float* __restrict__ tsdf, const unsigned char* __restrict__ cell, Grid g,
                                                            unsigned char* __restrict__ vertex_mask, uint32_t* __restrict__ vertex_counters,
                                                            uint32_t* __restrict__ triangle_counters) {
    __shared__ uint32_t lds[kWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t mine = 0;
#pragma unroll 1
    for (int r = 0; r < kRounds; ++r) {
        const long long n = tile_position(blockIdx.x, wave, r, lane);
        if (n >= g.nodes) continue;
        const unsigned char mask = (unsigned char)edge_mask(tsdf, cell, g, n);
        vertex_mask[n] = mask;
        mine += packed_counts(mask, cell[n]);
    }
    uint32_t total;
    block_exclusive_add(mine, lds, &total);
    if (threadIdx.x == 0) {
        vertex_counters[blockIdx.x] = total & 0xFFFFu;
        triangle_counters[blockIdx.x] = total >> 16;
    }
}

// grid (tiles): counters scanned.  first_vertex[n], first_triangle[n] of every node of the tile, in index order; counts[0 .. 1]
__global__ void __launch_bounds__(kBlock) mesh_firsts_kernel(const unsigned char* __restrict__ vertex_mask, const unsigned char* __restrict__ cell,
                                                             long long nodes, const uint32_t* __restrict__ vertex_counters,
                                                             const uint32_t* __restrict__ triangle_counters,
                                                             uint32_t* __restrict__ first_vertex, uint32_t* __restrict__ first_triangle,
                                                             long long* __restrict__ counts) {
    __shared__ uint32_t wave_total[kWaves];
    const long long tile = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t before[kRounds], held = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const long long n = tile_position(tile, wave, r, lane);
        const uint32_t mine = n < nodes ? packed_counts(vertex_mask[n], cell[n]) : 0u;
        const uint32_t inclusive = wave_inclusive_add_u32(mine);
        before[r] = held + inclusive - mine;
        held += __shfl(inclusive, kWave - 1, kWave);
    }
    if (lane == 0) wave_total[wave] = held;
    __syncthreads();
    uint32_t lower = 0, all = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        if (v < wave) lower += wave_total[v];
        all += wave_total[v];
    }
    const uint32_t vertex_base = vertex_counters[tile], triangle_base = triangle_counters[tile];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const long long n = tile_position(tile, wave, r, lane);
        if (n >= nodes) continue;
        const uint32_t at = lower + before[r];
        first_vertex[n] = vertex_base + (at & 0xFFFFu);
        first_triangle[n] = triangle_base + (at >> 16);
    }
    if (tile == (long long)gridDim.x - 1 && threadIdx.x == 0) {
        counts[0] = (long long)vertex_base + (all & 0xFFFFu);
        counts[1] = (long long)triangle_base + (all >> 16);
    }
}

// grid (ceil(nodes / kBlock)): the vertices of node n and the triangles of cell n.  Nothing is written at or past counts[].
__global__ void __launch_bounds__(kBlock) mesh_emit_kernel(const float* __restrict__ tsdf, Grid g, const unsigned char* __restrict__ cell,
                                                           const unsigned char* __restrict__ vertex_mask,
                                                           const uint32_t* __restrict__ first_vertex,
                                                           const uint32_t* __restrict__ first_triangle, const long long* __restrict__ counts,
                                                           float* __restrict__ vertices, int* __restrict__ triangles) {
    const long long n = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (n >= g.nodes) return;
    // (the guards on the indices below hold for a workspace that snerf_mesh_count filled for this grid; with any other, they keep
    // every read inside the arrays)
    int at[3];
    node_index(g, n, at);
    const unsigned mask = vertex_mask[n];
    if (mask) {
        const double t_a = (double)tsdf[n];
        long long to = first_vertex[n];
        const long long limit = counts[0];
        for (int type = 0; type < kKeysPerNode; ++type) {
            if (!((mask >> type) & 1u)) continue;
            const int code = kOffsetOfType[type];
            bool inside = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) inside = inside && at[a] + ((code >> a) & 1) < g.n[a];
            if (!inside) continue;
            const double t_b = (double)tsdf[neighbour(g, n, code)];
            const double s = t_a / (t_a - t_b);
            if (to < limit) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double p_a = g.lo[a] + g.voxel_size * (double)at[a];
                    const double p_b = g.lo[a] + g.voxel_size * (double)(at[a] + ((code >> a) & 1));
                    vertices[3 * to + a] = (float)(p_a + s * (p_b - p_a));
                }
            }
            ++to;
        }
    }
    const unsigned char c = cell[n];
    if (!(c & kComplete) || !(c & 0x7F)) return;
    if (!(at[0] < g.n[0] - 1 && at[1] < g.n[1] - 1 && at[2] < g.n[2] - 1)) return;
    const unsigned signs = cell_signs(tsdf, g, n);
    long long to = first_triangle[n];
    const long long limit = counts[1];
    for (int t = 0; t < kTetrahedra; ++t) {
        const TetCase entry = kTetCase[t][tetrahedron_case(signs, t)];
        for (int e = 0; e < 3 * entry.triangles; ++e) {
            const int code_a = kTetVertex[t][entry.edge[e] >> 2], code_b = kTetVertex[t][entry.edge[e] & 3];
            const long long a = neighbour(g, n, code_a);
            const int type = kTypeOfOffset[code_a ^ code_b];
            const long long row = to + e / 3;
            if (row < limit) triangles[3 * row + e % 3] = (int)(first_vertex[a] + (uint32_t)__popc((unsigned)vertex_mask[a] & ((1u << type) - 1u)));
        }
        to += entry.triangles;
    }
}

// the workspace of the extraction: [cell bytes | vertex masks | first vertices | first triangles | vertex counters | triangle
// counters], each part 256-byte aligned
struct MeshWorkspace {
    long long cell_offset, mask_offset, first_vertex_offset, first_triangle_offset, vertex_counters_offset, triangle_counters_offset, bytes, tiles;
    explicit MeshWorkspace(long long nodes) {
        tiles = snerf::sortplan::tiles(nodes);
        cell_offset = 0;
        mask_offset = cell_offset + align_up(nodes);
        first_vertex_offset = mask_offset + align_up(nodes);
        first_triangle_offset = first_vertex_offset + align_up(nodes * 4);
        vertex_counters_offset = first_triangle_offset + align_up(nodes * 4);
        triangle_counters_offset = vertex_counters_offset + align_up(tiles * 4);
        bytes = triangle_counters_offset + align_up(tiles * 4);
    }
};

// SNERF_OK with *f's extents filled, or the status the call returns (message set)
int views_of(const char* what, int views, int height, int width, Views* f) {
    SNERF_REQUIRE(views >= 0 && height >= 0 && width >= 0, "%s: %d views of %d x %d", what, views, height, width);
    SNERF_REQUIRE(views <= SNERF_FUSE_MAX_VIEWS, "%s: %d views, at most %d", what, views, SNERF_FUSE_MAX_VIEWS);
    const long long pixels = (long long)height * width;
    if (views > 0 && pixels > kMaxCount / views)
        return snerf::fail(SNERF_E_UNSUPPORTED, "%s: %d views of %d x %d exceed 2^31 - 1 pixels", what, views, height, width);
    f->views = pixels > 0 ? views : 0;     // (frames without pixels are looked up by nobody)
    f->height = height;
    f->width = width;
    f->pixels = pixels;
    return SNERF_OK;
}

int mesh_arguments(const char* what, const float* tsdf, const unsigned char* weight, int min_weight, const long long* counts,
                   const void* workspace) {
    SNERF_REQUIRE(min_weight >= 1 && min_weight <= 255, "%s: min_weight %d outside 1..255", what, min_weight);
    SNERF_REQUIRE(tsdf && weight && counts && workspace, "%s: NULL pointer", what);
    SNERF_REQUIRE(((unsigned long long)workspace & (kAlign - 1)) == 0, "%s: workspace must be 256-byte aligned", what);
    SNERF_REQUIRE(((unsigned long long)counts & 7) == 0, "%s: counts must be 8-byte aligned", what);
    return SNERF_OK;
}

}  // namespace

extern "C" int snerf_tsdf_integrate(const float* depth, const unsigned char* mask, const double* cameras, int views, int height, int width,
                                    double voxel_size, double lo_x, double lo_y, double lo_z, int nx, int ny, int nz, double truncation,
                                    float* tsdf, unsigned char* weight, snerf_stream_t stream) {
    Views f;
    int status = views_of("tsdf_integrate", views, height, width, &f);
    if (status != SNERF_OK) return status;
    Grid g;
    status = grid_of("tsdf_integrate", voxel_size, lo_x, lo_y, lo_z, nx, ny, nz, &g);
    if (status != SNERF_OK) return status;
    SNERF_REQUIRE(truncation > 0.0 && std::isfinite(truncation), "tsdf_integrate: truncation %g, expected a finite number > 0", truncation);
    SNERF_REQUIRE(tsdf && weight, "tsdf_integrate: NULL pointer");
    SNERF_REQUIRE(f.views == 0 || (depth && cameras), "tsdf_integrate: NULL pointer");
    f.depth = depth; f.mask = mask; f.cameras = cameras;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(node_blocks(g.nodes)), dim3(kBlock), 0, (hipStream_t)stream, f, g, truncation, tsdf, weight);
    return snerf::check_launch("tsdf_integrate");
}

extern "C" long long snerf_mesh_workspace_bytes(int nx, int ny, int nz) {
    Grid g;
    if (grid_of("mesh_workspace_bytes", 1.0, 0.0, 0.0, 0.0, nx, ny, nz, &g) != SNERF_OK) return 0;
    return MeshWorkspace(g.nodes).bytes;
}

extern "C" int snerf_mesh_count(const float* tsdf, const unsigned char* weight, double voxel_size, double lo_x, double lo_y, double lo_z,
                                int nx, int ny, int nz, int min_weight, long long* counts, void* workspace, snerf_stream_t stream) {
    Grid g;
    int status = grid_of("mesh_count", voxel_size, lo_x, lo_y, lo_z, nx, ny, nz, &g);
    if (status != SNERF_OK) return status;
    status = mesh_arguments("mesh_count", tsdf, weight, min_weight, counts, workspace);
    if (status != SNERF_OK) return status;
    const MeshWorkspace ws(g.nodes);
    char* base = (char*)workspace;
    unsigned char* cell = (unsigned char*)(base + ws.cell_offset);
    unsigned char* vertex_mask = (unsigned char*)(base + ws.mask_offset);
    uint32_t* first_vertex = (uint32_t*)(base + ws.first_vertex_offset);
    uint32_t* first_triangle = (uint32_t*)(base + ws.first_triangle_offset);
    uint32_t* vertex_counters = (uint32_t*)(base + ws.vertex_counters_offset);
    uint32_t* triangle_counters = (uint32_t*)(base + ws.triangle_counters_offset);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_cells_kernel, dim3(node_blocks(g.nodes)), dim3(kBlock), 0, s, tsdf, weight, g, min_weight, cell);
    hipLaunchKernelGGL(mesh_edges_kernel, dim3((unsigned)ws.tiles), dim3(kBlock), 0, s, tsdf, (const unsigned char*)cell, g, vertex_mask,
                       vertex_counters, triangle_counters);
    hipLaunchKernelGGL(scan_counters_kernel, dim3(1), dim3(kBlock), 0, s, vertex_counters, ws.tiles);
    hipLaunchKernelGGL(scan_counters_kernel, dim3(1), dim3(kBlock), 0, s, triangle_counters, ws.tiles);
    hipLaunchKernelGGL(mesh_firsts_kernel, dim3((unsigned)ws.tiles), dim3(kBlock), 0, s, (const unsigned char*)vertex_mask,
                       (const unsigned char*)cell, g.nodes, (const uint32_t*)vertex_counters, (const uint32_t*)triangle_counters, first_vertex,
                       first_triangle, counts);
    return snerf::check_launch("mesh_count");
}

extern "C" int snerf_mesh_emit(const float* tsdf, const unsigned char* weight, double voxel_size, double lo_x, double lo_y, double lo_z,
                               int nx, int ny, int nz, int min_weight, const long long* counts, float* vertices, int* triangles,
                               void* workspace, snerf_stream_t stream) {
    Grid g;
    int status = grid_of("mesh_emit", voxel_size, lo_x, lo_y, lo_z, nx, ny, nz, &g);
    if (status != SNERF_OK) return status;
    status = mesh_arguments("mesh_emit", tsdf, weight, min_weight, counts, workspace);
    if (status != SNERF_OK) return status;
    SNERF_REQUIRE(vertices && triangles, "mesh_emit: NULL pointer");
    const MeshWorkspace ws(g.nodes);
    const char* base = (const char*)workspace;
    hipLaunchKernelGGL(mesh_emit_kernel, dim3(node_blocks(g.nodes)), dim3(kBlock), 0, (hipStream_t)stream, tsdf, g,
                       (const unsigned char*)(base + ws.cell_offset), (const unsigned char*)(base + ws.mask_offset),
                       (const uint32_t*)(base + ws.first_vertex_offset), (const uint32_t*)(base + ws.first_triangle_offset), counts, vertices,
                       triangles);
    return snerf::check_launch("mesh_emit");
}

extern "C" int snerf_colour_points(const float* points, long long count, const float* depth, const unsigned char* image,
                                   const unsigned char* mask, const double* cameras, int views, int height, int width,
                                   double colour_tolerance, unsigned char* colours, unsigned char* agreeing, snerf_stream_t stream) {
    SNERF_REQUIRE(count >= 0, "colour_points: count %lld", count);
    Views f;
    const int status = views_of("colour_points", views, height, width, &f);
    if (status != SNERF_OK) return status;
    SNERF_REQUIRE(colour_tolerance >= 0.0, "colour_points: colour_tolerance %g, expected a number >= 0", colour_tolerance);
    if (count > kMaxCount) return snerf::fail(SNERF_E_UNSUPPORTED, "colour_points: count %lld exceeds 2^31 - 1", count);
    if (count == 0) return SNERF_OK;
    SNERF_REQUIRE(points && colours && agreeing, "colour_points: NULL pointer");
    SNERF_REQUIRE(f.views == 0 || (depth && image && cameras), "colour_points: NULL pointer");
    f.depth = depth; f.mask = mask; f.cameras = cameras;
    hipLaunchKernelGGL(colour_points_kernel, dim3(node_blocks(count)), dim3(kBlock), 0, (hipStream_t)stream, points, count, f, image,
                       colour_tolerance, colours, agreeing);
    return snerf::check_launch("colour_points");
}
