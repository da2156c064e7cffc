// snerf_png_deflate (simplenerf_png.h): 8-bit frames on the device -> the zlib stream of each frame's IDAT chunk.  Four launches:
//   filter  a workgroup per row: the five filter types' costs, the choice, the filtered row        (3 B read, 1 B written per byte)
//   code    a workgroup per 32 KiB strip of filtered bytes: run-length tokens, a Huffman code of the strip's own counts, the bits
//           assembled in LDS and written 16 bytes per lane -- or the strip as a stored block when that is not smaller
//   scan    a workgroup per frame: the strips' byte offsets, the zlib header, the Adler-32
//   pack    a workgroup per strip: its bytes to their offset in the frame's stream
// The workgroup programs are in png_coder.h, written so that a host program runs the same text (tests/native/png_coder_host.cpp).
// Bound: the code kernel's serial steps (one thread merges the <= 286 leaves of the Huffman tree); a frame of 2.3 MB is 70 strips.
#include "snerf_common.h"
#include "simplenerf_png.h"
#include "png_coder.h"

namespace {

namespace png = snerf::png;

static_assert(SNERF_PNG_STRIP_BYTES == png::kStrip, "the header's strip size is the coder's");
static_assert(sizeof(png::StripShared) <= 80 * 1024, "two strips per CU: 2 x 80 KiB of the 160 KiB of LDS");

struct Plan {
    int row_bytes, raw, strips;
    size_t stride;        // of a frame's filtered bytes: raw rounded up to 16, so that every strip starts 16-byte aligned
};

// false: the arguments are not an image this encoder takes
bool plan_of(int height, int width, int channels, Plan* plan) {
    if ((channels != 1 && channels != 3) || height < 1 || width < 1) return false;
    const long long row_bytes = (long long)width * channels, raw = (long long)height * (1 + row_bytes);
    if (raw >= (1ll << 31)) return false;
    plan->row_bytes = (int)row_bytes;
    plan->raw = (int)raw;
    plan->strips = (int)((raw + png::kStrip - 1) / png::kStrip);
    plan->stride = ((size_t)raw + 15) / 16 * 16;
    return true;
}

size_t bound_of(const Plan& plan) { return (size_t)plan.raw + 5 * (size_t)plan.strips + 6; }

// the workspace: [filtered bytes | coded strips | strip offsets | strip sizes | strip Adler pairs], each part 16-byte aligned
struct Workspace {
    unsigned char *filtered, *slots;
    long long* offsets;
    int* sizes;
    uint32_t* adler;
    size_t bytes;
    Workspace(void* base, int images, const Plan& plan) {
        const size_t strips = (size_t)images * plan.strips;
        auto round16 = [](size_t n) { return (n + 15) / 16 * 16; };
        size_t at = 0;
        auto take = [&](size_t n) {
            unsigned char* p = reinterpret_cast<unsigned char*>(reinterpret_cast<uintptr_t>(base) + at);
            at += round16(n);
            return p;
        };
        filtered = take((size_t)images * plan.stride);
        slots = take(strips * png::kSlot);
        offsets = reinterpret_cast<long long*>(take(strips * sizeof(long long)));
        sizes = reinterpret_cast<int*>(take(strips * sizeof(int)));
        adler = reinterpret_cast<uint32_t*>(take(strips * 2 * sizeof(uint32_t)));
        bytes = at;
    }
};

__global__ void __launch_bounds__(png::kThreads) png_filter_kernel(const unsigned char* __restrict__ pixels, int height, int row_bytes,
                                                                   int bpp, int mode, size_t stride, unsigned char* __restrict__ filtered) {
    __shared__ png::FilterShared sh;
    const int image = blockIdx.x / height, row = blockIdx.x - image * height;
    const unsigned char* cur = pixels + ((size_t)image * height + row) * row_bytes;
    png::filter_row(sh, cur, row ? cur - row_bytes : nullptr, row_bytes, bpp, mode,
                    filtered + (size_t)image * stride + (size_t)row * (1 + row_bytes));
}

__global__ void __launch_bounds__(png::kThreads) png_code_kernel(const unsigned char* __restrict__ filtered, int raw, int strips,
                                                                 size_t stride, unsigned char* __restrict__ slots,
                                                                 int* __restrict__ sizes, uint32_t* __restrict__ adler) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    png::StripShared& sh = *reinterpret_cast<png::StripShared*>(lds);
    const int image = blockIdx.x / strips, strip = blockIdx.x - image * strips;
    const int left = raw - strip * png::kStrip, length = left < png::kStrip ? left : png::kStrip;
    png::encode_strip(sh, filtered + (size_t)image * stride + (size_t)strip * png::kStrip, length, strip == strips - 1,
                      slots + (size_t)blockIdx.x * png::kSlot, sizes + blockIdx.x, adler + 2 * (size_t)blockIdx.x);
}

__global__ void __launch_bounds__(png::kThreads) png_scan_kernel(const int* __restrict__ sizes, const uint32_t* __restrict__ adler,
                                                                 int strips, int raw, long long* __restrict__ offsets,
                                                                 unsigned char* __restrict__ streams, size_t bound,
                                                                 long long* __restrict__ stream_bytes) {
    __shared__ png::ScanShared sh;
    const size_t first = (size_t)blockIdx.x * strips;
    png::scan_frame(sh, sizes + first, adler + 2 * first, strips, raw, offsets + first, streams + blockIdx.x * bound,
                    stream_bytes + blockIdx.x);
}

__global__ void __launch_bounds__(png::kThreads) png_pack_kernel(const unsigned char* __restrict__ slots, const int* __restrict__ sizes,
                                                                 const long long* __restrict__ offsets, int strips,
                                                                 unsigned char* __restrict__ streams, size_t bound) {
    const int image = blockIdx.x / strips;
    png::pack_strip(slots + (size_t)blockIdx.x * png::kSlot, sizes[blockIdx.x], streams + image * bound + offsets[blockIdx.x]);
}

}  // namespace

extern "C" size_t snerf_png_deflate_bound_bytes(int height, int width, int channels) {
    Plan plan;
    return plan_of(height, width, channels, &plan) ? bound_of(plan) : 0;
}

extern "C" size_t snerf_png_deflate_workspace_bytes(int images, int height, int width, int channels) {
    Plan plan;
    if (images < 1 || !plan_of(height, width, channels, &plan)) return 0;
    return Workspace(nullptr, images, plan).bytes;
}

extern "C" int snerf_png_deflate(const unsigned char* pixels, int images, int height, int width, int channels, int filter_mode,
                                 unsigned char* streams, long long* stream_bytes, void* workspace, snerf_stream_t stream) {
    Plan plan;
    SNERF_REQUIRE(channels == 1 || channels == 3, "png_deflate: channels %d, expected 1 or 3", channels);
    SNERF_REQUIRE(height >= 1 && width >= 1, "png_deflate: height %d, width %d", height, width);
    SNERF_REQUIRE(filter_mode >= SNERF_PNG_FILTER_ADAPTIVE && filter_mode <= 4, "png_deflate: filter_mode %d outside -1..4", filter_mode);
    SNERF_REQUIRE(plan_of(height, width, channels, &plan), "png_deflate: %d x %d x %d has 2^31 filtered bytes or more", height, width,
                  channels);
    SNERF_REQUIRE(images >= 0, "png_deflate: images %d", images);
    if (images == 0) return SNERF_OK;
    SNERF_REQUIRE(pixels && streams && stream_bytes && workspace, "png_deflate: NULL pointer");
    SNERF_REQUIRE(((unsigned long long)workspace & 15) == 0, "png_deflate: workspace must be 16-byte aligned");
    if ((long long)images * height > 0x7fffffffLL || (long long)images * plan.strips > 0x7fffffffLL)
        return snerf::fail(SNERF_E_UNSUPPORTED, "png_deflate: %d images of %d rows are too many for one call", images, height);
    static snerf::DeviceOnce configured;
    const int attr = snerf::raise_dynamic_lds(configured, reinterpret_cast<const void*>(png_code_kernel), (int)sizeof(png::StripShared),
                                              "png_deflate");
    if (attr != SNERF_OK) return attr;
    const Workspace ws(workspace, images, plan);
    const size_t bound = bound_of(plan);
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(png::kThreads);
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)(images * height)), block, 0, s, pixels, height, plan.row_bytes, channels,
                       filter_mode, plan.stride, ws.filtered);
    hipLaunchKernelGGL(png_code_kernel, dim3((unsigned)(images * plan.strips)), block, sizeof(png::StripShared), s, ws.filtered,
                       plan.raw, plan.strips, plan.stride, ws.slots, ws.sizes, ws.adler);
    hipLaunchKernelGGL(png_scan_kernel, dim3((unsigned)images), block, 0, s, ws.sizes, ws.adler, plan.strips, plan.raw, ws.offsets,
                       streams, bound, stream_bytes);
    hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)(images * plan.strips)), block, 0, s, ws.slots, ws.sizes, ws.offsets,
                       plan.strips, streams, bound);
    return snerf::check_launch("png_deflate");
}
