// Output post-processing on the device: what the reference's Tester does on the host after copying
// every fp32 output back -- post_process_image / post_process_depth (src/data_preprocessors/DataPreprocessor01.py
// :1106-1114): colour -> clip to [0,1] -> round(255 x) (round-half-to-even, as numpy.round) -> uint8; depth -> clip at 0.
// One pass, 16 B read and 7 B written per ray, so a frame leaves the GPU as 3 B/pixel instead of 12 (+ ~1 KB/ray of
// alpha the reference also ships).  Bound: HBM.
#include "snerf_common.h"
#include "block_reduce.h"
#include "simplenerf_maps.h"

namespace {

namespace reduce = snerf::reduce;

__global__ void __launch_bounds__(256) to_display_kernel(const float* __restrict__ rgb, const float* __restrict__ depth,
                                                         long long n, unsigned char* __restrict__ image,
                                                         float* __restrict__ depth_out) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
#pragma unroll
        for (int c = 0; c < 3 && image; ++c) {
            float v = rgb[3 * i + c];
            // numpy.clip, then round-half-to-even, then the uint8 cast.  NaN: numpy keeps it through clip and round and
            // its float->uint8 cast yields 0 on x86-64 (pinned by tests/golden/display.npz); fmaxf(NaN, 0) = 0 gives the
            // same byte here
            v = fminf(fmaxf(v, 0.0f), 1.0f);
            image[3 * i + c] = (unsigned char)rintf(v * 255.0f);
        }
        if (depth_out) {
            // numpy.clip(depth, 0, inf): comparisons, not fmaxf -- NaN stays NaN and -0.0 stays -0.0 as in the reference
            const float d = depth[i];
            depth_out[i] = d < 0.0f ? 0.0f : d;
        }
    }
}

// ---- snerf_maps_to_u8: the trainer's 8-bit previews.  Two launches over a (blocks, map) grid: the maps' maxima as per-workgroup
// partials (4 B read per value), then every workgroup folds its map's <= kMaxPartials partials (L2) and converts (4 B read, 1 B
// written).  Bound: HBM.  Each map is walked as [<= 3 values | 16-byte vectors | <= 3 values] from its own first 16-byte boundary.
constexpr int kMaxPartials = 128;      // <= reduce::kBlock: the second launch reads one partial per thread
constexpr long long kValuesPerBlock = 4ll * 4 * reduce::kBlock;     // four 16-byte loads per thread before a map gets another workgroup

// numpy.maximum: a NaN on either side stays
struct NanMax {
    __device__ __forceinline__ float operator()(float a, float b) const { return a != a ? a : ((b > a || b != b) ? b : a); }
};
constexpr NanMax nan_max{};

struct MapWalk {
    long long head, vectors, edges;     // values before the first 16-byte boundary; float4 after it; head + tail values (<= 6)
    __device__ MapWalk(const float* map, long long n) {
        const long long to_boundary = (long long)((16 - ((unsigned long long)map & 15)) & 15) >> 2;
        head = to_boundary < n ? to_boundary : n;
        vectors = (n - head) >> 2;
        edges = n - 4 * vectors;
    }
    // position in the map of edge value j (0 <= j < edges)
    __device__ long long edge(long long j) const { return j < head ? j : j + 4 * vectors; }
};

__global__ void __launch_bounds__(reduce::kBlock) maps_max_kernel(const float* __restrict__ maps, const int* __restrict__ modes,
                                                                  long long n, float* __restrict__ partials) {
    __shared__ float lds[reduce::kWaves];
    const int k = blockIdx.y;
    if (modes[k] == 0) return;          // (uniform over the workgroup)
    const float* map = maps + (long long)k * n;
    const MapWalk walk(map, n);
    const float4* body = reinterpret_cast<const float4*>(map + walk.head);
    const long long first = (long long)blockIdx.x * reduce::kBlock + threadIdx.x, stride = (long long)gridDim.x * reduce::kBlock;
    float m = -INFINITY;
    for (long long i = first; i < walk.vectors; i += stride) {
        const float4 v = body[i];
        m = nan_max(m, nan_max(nan_max(v.x, v.y), nan_max(v.z, v.w)));
    }
    for (long long j = first; j < walk.edges; j += stride) m = nan_max(m, map[walk.edge(j)]);
    m = reduce::block_fold(m, lds, nan_max);
    if (threadIdx.x == 0) partials[(long long)k * gridDim.x + blockIdx.x] = m;
}

// one value of a map whose status is 0: `scaled` divides by the map's maximum first
__device__ __forceinline__ unsigned char to_u8(float x, float maximum, bool scaled) {
    const float r = rintf((scaled ? x / maximum : x) * 255.0f);
    return (unsigned char)fminf(fmaxf(r, 0.0f), 255.0f);      // fmaxf(NaN, 0) = 0
}

__global__ void __launch_bounds__(reduce::kBlock) maps_convert_kernel(const float* __restrict__ maps, const int* __restrict__ modes,
                                                                      long long n, const float* __restrict__ partials,
                                                                      unsigned char* __restrict__ out, int* __restrict__ status) {
    __shared__ float lds[reduce::kWaves];
    const int k = blockIdx.y;
    const int mode = modes[k];
    const bool scaled = mode != 0;
    float maximum = 1.0f;
    int bad = 0;
    if (scaled) {
        // (the first launch ran on this launch's grid: gridDim.x partials per map)
        const float p = threadIdx.x < gridDim.x ? partials[(long long)k * gridDim.x + threadIdx.x] : -INFINITY;
        maximum = reduce::block_fold(p, lds, nan_max);
        bad = mode != 1 ? 2 : (maximum > 0.0f && maximum < INFINITY ? 0 : 1);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) status[k] = bad;
    const float* map = maps + (long long)k * n;
    unsigned char* bytes = out + (long long)k * n;
    const MapWalk walk(map, n);
    const float4* body = reinterpret_cast<const float4*>(map + walk.head);
    const bool wide_store = (((unsigned long long)(bytes + walk.head)) & 3) == 0;
    const long long first = (long long)blockIdx.x * reduce::kBlock + threadIdx.x, stride = (long long)gridDim.x * reduce::kBlock;
    for (long long i = first; i < walk.vectors; i += stride) {
        uchar4 b = make_uchar4(0, 0, 0, 0);
        if (!bad) {
            const float4 v = body[i];
            b = make_uchar4(to_u8(v.x, maximum, scaled), to_u8(v.y, maximum, scaled), to_u8(v.z, maximum, scaled),
                            to_u8(v.w, maximum, scaled));
        }
        unsigned char* at = bytes + walk.head + 4 * i;
        if (wide_store) {
            *reinterpret_cast<uchar4*>(at) = b;
        } else {
            at[0] = b.x, at[1] = b.y, at[2] = b.z, at[3] = b.w;
        }
    }
    for (long long j = first; j < walk.edges; j += stride) {
        const long long at = walk.edge(j);
        bytes[at] = bad ? (unsigned char)0 : to_u8(map[at], maximum, scaled);
    }
}

}  // namespace

extern "C" long long snerf_maps_to_u8_workspace_bytes(int num_maps) {
    return num_maps > 0 ? (long long)num_maps * kMaxPartials * (long long)sizeof(float) : 0;
}

extern "C" int snerf_maps_to_u8(const float* maps, const int* modes, int num_maps, long long n, unsigned char* out, int* status,
                                void* workspace, snerf_stream_t stream) {
    SNERF_REQUIRE(num_maps >= 0 && num_maps <= 65535, "maps_to_u8: num_maps %d outside 0..65535", num_maps);
    SNERF_REQUIRE(n >= 0, "maps_to_u8: negative map size");
    if (num_maps == 0 || n == 0) return SNERF_OK;
    SNERF_REQUIRE(maps && modes && out && status && workspace, "maps_to_u8: NULL pointer");
    SNERF_REQUIRE(((unsigned long long)maps & 3) == 0, "maps_to_u8: maps must be 4-byte aligned");
    long long blocks = (n + kValuesPerBlock - 1) / kValuesPerBlock;
    if (blocks > kMaxPartials) blocks = kMaxPartials;
    const dim3 grid((unsigned)blocks, (unsigned)num_maps);
    hipLaunchKernelGGL(maps_max_kernel, grid, dim3(reduce::kBlock), 0, (hipStream_t)stream, maps, modes, n, (float*)workspace);
    hipLaunchKernelGGL(maps_convert_kernel, grid, dim3(reduce::kBlock), 0, (hipStream_t)stream, maps, modes, n,
                       (const float*)workspace, out, status);
    return snerf::check_launch("maps_to_u8");
}

extern "C" int snerf_to_display(const float* rgb, const float* depth, long long num_rays, unsigned char* image,
                                float* depth_out, snerf_stream_t stream) {
    SNERF_REQUIRE((rgb && image) || (!image && depth_out), "to_display: NULL pointer");
    SNERF_REQUIRE(!depth_out || depth, "to_display: depth_out requested without depth");
    SNERF_REQUIRE(num_rays >= 0, "to_display: negative ray count");
    if (num_rays == 0) return SNERF_OK;
    hipLaunchKernelGGL(to_display_kernel, dim3(snerf::stride_grid(num_rays, 256)), dim3(256), 0, (hipStream_t)stream, rgb,
                       depth, num_rays, image, depth_out);
    return snerf::check_launch("to_display");
}
