// The geometry export (simplenerf_fuse.h): depth maps on the device -> one consistency-filtered, coloured point cloud, and its thinning
// to one point per occupied voxel.
//
// snerf_fuse_depth_maps, four launches:
//   decide   a workgroup per tile of 2048 pixels (sort_plan.h's tiling: wave, round, lane IS the index order): a thread unprojects
//            its pixels, reprojects each into the other views, counts the views that agree, stores one state byte per pixel (0:
//            dropped, else agreeing views + 1) and the tile's number of kept pixels
//   scan     one workgroup scans the tile counters exclusively, chunk after chunk with a running carry
//   scatter  a workgroup per tile: ballots rank the kept pixels of a round, the rounds and waves before them add up to the position
//            in the tile; the point is computed again (the same expression: the same bits) and written with its colour and count
// snerf_voxel_thin: keys -> snerf_sort_keys_with_order (sort.hip) -> the same count / scan / scatter on the run heads of the sorted
// keys, the scattering thread walking its run.
// No atomics: every position comes from counts and scans in index order, so the same input gives the same bits.  fp64 throughout
// (the library is built with -ffp-contract=off: no product is fused into a sum).
// Bound: decide by the fp64 divide rate and the views - 1 dependent depth reads per pixel, the rest by memory latency; the thinning by
// its sort, and by the longest run (one thread sums it in order, as the rule says).
#include <cfloat>
#include <cmath>

#include "snerf_common.h"
#include "simplenerf_fuse.h"
#include "fuse_point.h"
#include "sort_plan.h"
#include "tile_scan.h"

namespace {

using namespace snerf::sortplan;
using namespace snerf::tilescan;

using namespace snerf::fusepoint;      // the camera row's offsets, valid_depth, affine, unproject: shared with normals.hip

struct Frames {
    const float* depth;
    const unsigned char* image;
    const unsigned char* mask;      // or NULL
    const double* cameras;
    int views, height, width;
    long long pixels;               // height * width
    long long total;                // views * pixels
};

__device__ __forceinline__ bool valid_pixel(const Frames& f, long long i) {
    return valid_depth(f.depth[i]) && (!f.mask || f.mask[i] != 0);
}

// The state byte of pixel i < total: 0 = not kept, else 1 + the number of agreeing views.
__device__ __forceinline__ unsigned char decide(const Frames& f, long long i, double tau, int min_views) {
    if (!valid_pixel(f, i)) return 0;
    const int v = (int)(i / f.pixels);
    const long long pixel = i - v * f.pixels;
    const int y = (int)(pixel / f.width), x = (int)(pixel - (long long)y * f.width);
    double P[3];
    unproject(f.cameras + (long long)v * kCamera, x, y, (double)f.depth[i], P);
    int agree = 0;
    for (int u = 0; u < f.views; ++u) {
        if (u == v) continue;
        const double* cam = f.cameras + (long long)u * kCamera;
        double c[3];
        affine(cam + kE, P, c);
        if (!(c[2] > 0.0)) continue;
        const double* K = cam + kK;
        const double q0 = (K[0] * c[0] + K[1] * c[1]) + K[2] * c[2];
        const double q1 = (K[3] * c[0] + K[4] * c[1]) + K[5] * c[2];
        const double q2 = (K[6] * c[0] + K[7] * c[1]) + K[8] * c[2];
        const double ix = rint(q0 / q2), iy = rint(q1 / q2);
        if (!(ix >= 0.0 && ix < (double)f.width && iy >= 0.0 && iy < (double)f.height)) continue;     // (a NaN fails every comparison)
        const long long j = (long long)u * f.pixels + (long long)iy * f.width + (long long)ix;
        if (!valid_pixel(f, j)) continue;
        const double du = (double)f.depth[j];
        if (fabs(c[2] - du) <= tau * du) ++agree;
    }
    return agree >= min_views ? (unsigned char)(agree + 1) : 0;
}

// ------------------------------------------------------------------------------------------------ fuse
// grid (tiles): state[i] of every pixel of the tile, counters[tile] = the tile's number of kept pixels
__global__ void __launch_bounds__(kBlock) fuse_decide_kernel(Frames f, double tau, int min_views, unsigned char* __restrict__ state,
                                                             uint32_t* __restrict__ counters) {
    __shared__ uint32_t lds[kWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t mine = 0;
#pragma unroll 1
    for (int r = 0; r < kRounds; ++r) {
        const long long i = tile_position(blockIdx.x, wave, r, lane);
        if (i >= f.total) continue;
        const unsigned char s = decide(f, i, tau, min_views);
        state[i] = s;
        mine += s != 0;
    }
    uint32_t total;
    block_exclusive_add(mine, lds, &total);
    if (threadIdx.x == 0) counters[blockIdx.x] = total;
}

// grid (tiles): counters scanned.  Kept pixel i goes to counters[tile] + its position among the tile's kept pixels.
__global__ void __launch_bounds__(kBlock) fuse_scatter_kernel(Frames f, const unsigned char* __restrict__ state,
                                                              const uint32_t* __restrict__ counters, float* __restrict__ points,
                                                              unsigned char* __restrict__ colours, unsigned char* __restrict__ agreeing,
                                                              long long* __restrict__ kept_count) {
    __shared__ uint32_t wave_total[kWaves];
    const long long tile = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned kept = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const long long i = tile_position(tile, wave, r, lane);
        if (i < f.total && state[i] != 0) kept |= 1u << r;
    }
    uint32_t rank[kRounds], start, all;
    tile_ranks(kept, wave_total, rank, &start, &all);
    const long long base = (long long)counters[tile] + start;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        if (!((kept >> r) & 1u)) continue;
        const long long i = tile_position(tile, wave, r, lane), to = base + rank[r];
        if (to >= f.total) continue;   // (cannot happen with counters of this state; never write outside the buffers)
        const int v = (int)(i / f.pixels);
        const long long pixel = i - v * f.pixels;
        const int y = (int)(pixel / f.width), x = (int)(pixel - (long long)y * f.width);
        double P[3];
        unproject(f.cameras + (long long)v * kCamera, x, y, (double)f.depth[i], P);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            points[3 * to + a] = (float)P[a];
            colours[3 * to + a] = f.image[3 * i + a];
        }
        agreeing[to] = (unsigned char)(state[i] - 1);
    }
    if (tile == (long long)gridDim.x - 1 && threadIdx.x == 0) kept_count[0] = (long long)counters[tile] + all;
}

// the workspace of the fuse: [state bytes | tile counters], each part 256-byte aligned
struct FuseWorkspace {
    long long state_offset, counters_offset, bytes, tiles;
    explicit FuseWorkspace(long long total) {
        tiles = snerf::sortplan::tiles(total);
        state_offset = 0;
        counters_offset = align_up(total);
        bytes = counters_offset + align_up(tiles * 4);
    }
};

// SNERF_OK with *total = views * height * width, or the status the call returns (message set)
int fuse_extent(int views, int height, int width, long long* total) {
    SNERF_REQUIRE(views >= 0 && height >= 0 && width >= 0, "fuse_depth_maps: %d views of %d x %d", views, height, width);
    SNERF_REQUIRE(views <= SNERF_FUSE_MAX_VIEWS, "fuse_depth_maps: %d views, at most %d", views, SNERF_FUSE_MAX_VIEWS);
    const long long pixels = (long long)height * width;     // (< 2^62)
    if (views > 0 && pixels > kMaxCount / views)
        return snerf::fail(SNERF_E_UNSUPPORTED, "fuse_depth_maps: %d views of %d x %d exceed 2^31 - 1 pixels", views, height, width);
    *total = pixels * views;
    return SNERF_OK;
}

// ------------------------------------------------------------------------------------------------ thin
struct Grid {
    double voxel_size, lo[3];
    int n[3];
};

__global__ void __launch_bounds__(kBlock) thin_keys_kernel(const float* __restrict__ points, long long count, Grid g, int* __restrict__ keys) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < count; i += stride) {
        long long cell[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double at = floor(((double)points[3 * i + a] - g.lo[a]) / g.voxel_size);
            cell[a] = at >= (double)g.n[a] ? g.n[a] - 1 : at >= 0.0 ? (long long)at : 0;     // (a NaN: 0)
        }
        keys[i] = (int)((cell[2] * g.n[1] + cell[1]) * g.n[0] + cell[0]);     // (< nx ny nz <= 2^31 - 1)
    }
}

// Bit r of the result: the calling lane's position of round r is inside `count` and begins a run of equal sorted keys.
__device__ __forceinline__ unsigned head_rounds(const int* __restrict__ sorted_keys, long long count, long long tile) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned heads = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const long long i = tile_position(tile, wave, r, lane);
        if (i < count && (i == 0 || sorted_keys[i] != sorted_keys[i - 1])) heads |= 1u << r;
    }
    return heads;
}

// grid (tiles): counters[tile] = the run heads of the tile
__global__ void __launch_bounds__(kBlock) thin_count_kernel(const int* __restrict__ sorted_keys, long long count, uint32_t* __restrict__ counters) {
    __shared__ uint32_t lds[kWaves];
    uint32_t total;
    block_exclusive_add((uint32_t)__popc(head_rounds(sorted_keys, count, blockIdx.x)), lds, &total);
    if (threadIdx.x == 0) counters[blockIdx.x] = total;
}

// grid (tiles): counters scanned.  The thread of a run head walks its run (which may leave the tile) in sorted = ascending source
// order and writes the run at its number.
__global__ void __launch_bounds__(kBlock) thin_runs_kernel(const float* __restrict__ points, const unsigned char* __restrict__ colours,
                                                           const int* __restrict__ sorted_keys, const long long* __restrict__ order,
                                                           long long count, const uint32_t* __restrict__ counters,
                                                           float* __restrict__ thinned_points, unsigned char* __restrict__ thinned_colours,
                                                           int* __restrict__ counts, long long* __restrict__ runs) {
    __shared__ uint32_t wave_total[kWaves];
    const long long tile = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const unsigned heads = head_rounds(sorted_keys, count, tile);
    uint32_t rank[kRounds], start, all;
    tile_ranks(heads, wave_total, rank, &start, &all);
    const long long base = (long long)counters[tile] + start;
#pragma unroll 1
    for (int r = 0; r < kRounds; ++r) {
        if (!((heads >> r) & 1u)) continue;
        const long long i = tile_position(tile, wave, r, lane), to = base + rank[r];
        if (to >= count) continue;   // (cannot happen with counters of these keys; never write outside the buffers)
        const int key = sorted_keys[i];
        double sum[3] = {0.0, 0.0, 0.0};
        unsigned long long colour[3] = {0ull, 0ull, 0ull};
        long long members = 0;
        for (long long j = i; j < count && sorted_keys[j] == key; ++j) {
            const long long source = order[j];
            if (source < 0 || source >= count) continue;   // (an `order` that is no permutation: never read outside the buffers)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                sum[a] += (double)points[3 * source + a];
                colour[a] += colours[3 * source + a];
            }
            ++members;
        }
        const unsigned long long m = members > 0 ? (unsigned long long)members : 1ull;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            thinned_points[3 * to + a] = (float)(sum[a] / (double)m);
            thinned_colours[3 * to + a] = (unsigned char)((2ull * colour[a] + m) / (2ull * m));
        }
        counts[to] = (int)members;
    }
    if (tile == (long long)gridDim.x - 1 && threadIdx.x == 0) runs[0] = (long long)counters[tile] + all;
}

__global__ void zero_runs_kernel(long long* runs) { runs[0] = 0; }

int key_bits_of(long long cells) {
    int bits = 1;
    while (bits < 32 && (1ll << bits) < cells) ++bits;
    return bits;
}

// the workspace of the thinning: [keys | sorted keys | order | tile counters | the sort's own], each part 256-byte aligned
struct ThinWorkspace {
    long long keys_offset, sorted_offset, order_offset, counters_offset, sort_offset, bytes, tiles;
    ThinWorkspace(long long count, int key_bits) {
        tiles = snerf::sortplan::tiles(count);
        keys_offset = 0;
        sorted_offset = keys_offset + align_up(count * 4);
        order_offset = sorted_offset + align_up(count * 4);
        counters_offset = order_offset + align_up(count * 8);
        sort_offset = counters_offset + align_up(tiles * 4);
        SortPlan plan;
        bytes = plan_sort(count, key_bits, plan) ? sort_offset + align_up(plan.bytes) : 0;
    }
};

// SNERF_OK with *cells = nx ny nz, or the status the call returns (message set)
int thin_extent(long long count, int nx, int ny, int nz, long long* cells) {
    SNERF_REQUIRE(count >= 0, "voxel_thin: count %lld", count);
    SNERF_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "voxel_thin: extents %d x %d x %d, each must be at least 1", nx, ny, nz);
    if (count > kMaxCount) return snerf::fail(SNERF_E_UNSUPPORTED, "voxel_thin: count %lld exceeds 2^31 - 1", count);
    const long long xy = (long long)nx * ny;
    if (xy > kMaxCount || xy * nz > kMaxCount)
        return snerf::fail(SNERF_E_UNSUPPORTED, "voxel_thin: extents %d x %d x %d exceed 2^31 - 1 voxels", nx, ny, nz);
    *cells = xy * nz;
    return SNERF_OK;
}

}  // namespace

extern "C" long long snerf_fuse_depth_maps_workspace_bytes(int views, int height, int width) {
    long long total = 0;
    if (fuse_extent(views, height, width, &total) != SNERF_OK || total == 0) return 0;
    return FuseWorkspace(total).bytes;
}

extern "C" int snerf_fuse_depth_maps(const float* depth, const unsigned char* image, const unsigned char* mask, const double* cameras,
                                     int views, int height, int width, double depth_error_threshold, int min_views, float* points,
                                     unsigned char* colours, unsigned char* agreeing, long long* kept, void* workspace,
                                     snerf_stream_t stream) {
    long long total = 0;
    const int status = fuse_extent(views, height, width, &total);
    if (status != SNERF_OK) return status;
    SNERF_REQUIRE(depth_error_threshold >= 0.0, "fuse_depth_maps: depth_error_threshold %g, expected a number >= 0", depth_error_threshold);
    SNERF_REQUIRE(min_views >= 0 && min_views <= (views > 0 ? views - 1 : 0), "fuse_depth_maps: min_views %d outside 0..%d (the other views)",
                  min_views, views > 0 ? views - 1 : 0);
    if (total == 0) return SNERF_OK;
    SNERF_REQUIRE(depth && image && cameras && points && colours && agreeing && kept && workspace, "fuse_depth_maps: NULL pointer");
    SNERF_REQUIRE(((unsigned long long)workspace & (kAlign - 1)) == 0, "fuse_depth_maps: workspace must be 256-byte aligned");
    SNERF_REQUIRE(((unsigned long long)kept & 7) == 0, "fuse_depth_maps: kept must be 8-byte aligned");
    const FuseWorkspace ws(total);
    unsigned char* state = (unsigned char*)workspace + ws.state_offset;
    uint32_t* counters = (uint32_t*)((char*)workspace + ws.counters_offset);
    Frames f;
    f.depth = depth; f.image = image; f.mask = mask; f.cameras = cameras;
    f.views = views; f.height = height; f.width = width;
    f.pixels = (long long)height * width;
    f.total = total;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fuse_decide_kernel, dim3((unsigned)ws.tiles), dim3(kBlock), 0, s, f, depth_error_threshold, min_views, state, counters);
    hipLaunchKernelGGL(scan_counters_kernel, dim3(1), dim3(kBlock), 0, s, counters, ws.tiles);
    hipLaunchKernelGGL(fuse_scatter_kernel, dim3((unsigned)ws.tiles), dim3(kBlock), 0, s, f, (const unsigned char*)state,
                       (const uint32_t*)counters, points, colours, agreeing, kept);
    return snerf::check_launch("fuse_depth_maps");
}

extern "C" long long snerf_voxel_thin_workspace_bytes(long long count, int nx, int ny, int nz) {
    long long cells = 0;
    if (thin_extent(count, nx, ny, nz, &cells) != SNERF_OK || count == 0) return 0;
    return ThinWorkspace(count, key_bits_of(cells)).bytes;
}

extern "C" int snerf_voxel_thin(const float* points, const unsigned char* colours, long long count, double voxel_size, double lo_x,
                                double lo_y, double lo_z, int nx, int ny, int nz, float* thinned_points,
                                unsigned char* thinned_colours, int* counts, long long* runs, void* workspace, snerf_stream_t stream) {
    long long cells = 0;
    const int status = thin_extent(count, nx, ny, nz, &cells);
    if (status != SNERF_OK) return status;
    SNERF_REQUIRE(voxel_size > 0.0 && std::isfinite(voxel_size), "voxel_thin: voxel_size %g, expected a finite number > 0", voxel_size);
    SNERF_REQUIRE(std::isfinite(lo_x) && std::isfinite(lo_y) && std::isfinite(lo_z), "voxel_thin: the bound (%g, %g, %g) is not finite",
                  lo_x, lo_y, lo_z);
    SNERF_REQUIRE(runs, "voxel_thin: runs is NULL");
    SNERF_REQUIRE(((unsigned long long)runs & 7) == 0, "voxel_thin: runs must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (count == 0) {
        hipLaunchKernelGGL(zero_runs_kernel, dim3(1), dim3(1), 0, s, runs);
        return snerf::check_launch("voxel_thin");
    }
    SNERF_REQUIRE(points && colours && thinned_points && thinned_colours && counts && workspace, "voxel_thin: NULL pointer");
    SNERF_REQUIRE(((unsigned long long)workspace & (kAlign - 1)) == 0, "voxel_thin: workspace must be 256-byte aligned");
    const int key_bits = key_bits_of(cells);
    const ThinWorkspace ws(count, key_bits);
    SNERF_REQUIRE(ws.bytes > 0, "voxel_thin: count %lld cannot be planned", count);
    char* base = (char*)workspace;
    int* keys = (int*)(base + ws.keys_offset);
    int* sorted_keys = (int*)(base + ws.sorted_offset);
    long long* order = (long long*)(base + ws.order_offset);
    uint32_t* counters = (uint32_t*)(base + ws.counters_offset);
    Grid g;
    g.voxel_size = voxel_size;
    g.lo[0] = lo_x; g.lo[1] = lo_y; g.lo[2] = lo_z;
    g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
    hipLaunchKernelGGL(thin_keys_kernel, dim3(snerf::stride_grid(count, kBlock)), dim3(kBlock), 0, s, points, count, g, keys);
    // (every check the sort makes was made above: it cannot refuse after the first launch)
    const int sorted = snerf_sort_keys_with_order(keys, count, key_bits, sorted_keys, order, base + ws.sort_offset, stream);
    if (sorted != SNERF_OK) return sorted;
    hipLaunchKernelGGL(thin_count_kernel, dim3((unsigned)ws.tiles), dim3(kBlock), 0, s, (const int*)sorted_keys, count, counters);
    hipLaunchKernelGGL(scan_counters_kernel, dim3(1), dim3(kBlock), 0, s, counters, ws.tiles);
    hipLaunchKernelGGL(thin_runs_kernel, dim3((unsigned)ws.tiles), dim3(kBlock), 0, s, points, colours, (const int*)sorted_keys,
                       (const long long*)order, count, (const uint32_t*)counters, thinned_points, thinned_colours, counts, runs);
    return snerf::check_launch("voxel_thin");
}
