// snerf_jpeg_scan (simplenerf_jpeg.h): 8-bit frames on the device -> the entropy-coded segment of each frame's baseline JPEG scan.
// Three launches:
//   transform  a workgroup per chunk of 8 colour / 32 grey MCUs: colour conversion and 2 x 2 chroma means into LDS, the 8 x 8 DCT as
//              two integer matrix passes, quantised levels in zig-zag order as int16          (3 B read, 3 B written per pixel)
//   emit       a workgroup per MCU row (one restart interval): passes of 256 blocks, a thread per block -- bit counts, their scan,
//              the codes OR-ed into a bit buffer in LDS sized by the bound (256 x 208 B), then FF bytes counted, scanned and the
//              stuffed bytes written to the row's slot; the open bits of a pass are carried into the next
//   pack       a workgroup per MCU row: the sizes of the rows before it summed, its bytes copied to their offset in the frame's scan
// The workgroup programs are in jpeg_coder.h, written so that a host program runs the same text (tests/native/jpeg_coder_host.cpp).
// Bound: the emit kernel's serial steps (a thread walks the 64 levels of its block twice; one thread scans 256 counts).
#include "snerf_common.h"
#include "simplenerf_jpeg.h"
#include "jpeg_coder.h"

namespace {

namespace jpeg = snerf::jpeg;

static_assert(SNERF_JPEG_BLOCK_BYTES == jpeg::kBlockBytes, "the header's block bound is the coder's");
static_assert(sizeof(jpeg::EmitShared) <= 64 * 1024, "static LDS");
static_assert(jpeg::kColourChunkMcus * 6 <= jpeg::kChunkBlocks && jpeg::kGreyChunkMcus <= jpeg::kChunkBlocks, "a chunk's blocks fit");

struct Plan {
    int mcus_per_row, mcu_rows, blocks_per_row, chunk_mcus, chunks;
    size_t row_bound;          // bytes one MCU row can code to
    size_t row_stride;         // of a row's slot in the workspace: row_bound rounded up to 16
};

// false: the arguments are not an image this encoder takes
bool plan_of(int height, int width, int channels, Plan* plan) {
    if ((channels != 1 && channels != 3) || height < 1 || width < 1 || height > 65535 || width > 65535) return false;
    const int mcu = channels == 3 ? 16 : 8;
    plan->mcus_per_row = (width + mcu - 1) / mcu;
    plan->mcu_rows = (height + mcu - 1) / mcu;
    plan->blocks_per_row = plan->mcus_per_row * (channels == 3 ? 6 : 1);
    plan->chunk_mcus = channels == 3 ? jpeg::kColourChunkMcus : jpeg::kGreyChunkMcus;
    plan->chunks = (plan->mcus_per_row + plan->chunk_mcus - 1) / plan->chunk_mcus;
    plan->row_bound = 2 * (size_t)jpeg::kBlockBytes * plan->blocks_per_row + 2;
    plan->row_stride = (plan->row_bound + 15) / 16 * 16;
    return true;
}

size_t bound_of(const Plan& plan) { return (size_t)plan.mcu_rows * plan.row_bound; }

bool too_many(int images, const Plan& plan) { return (long long)images * plan.mcu_rows * plan.chunks > 0x7fffffffLL; }

// the workspace: [levels | row slots | row sizes], each part 16-byte aligned
struct Workspace {
    int16_t* levels;
    unsigned char* slots;
    int* sizes;
    size_t bytes;
    Workspace(void* base, int images, const Plan& plan) {
        const size_t rows = (size_t)images * plan.mcu_rows;
        auto round16 = [](size_t n) { return (n + 15) / 16 * 16; };
        size_t at = 0;
        auto take = [&](size_t n) {
            unsigned char* p = reinterpret_cast<unsigned char*>(reinterpret_cast<uintptr_t>(base) + at);
            at += round16(n);
            return p;
        };
        levels = reinterpret_cast<int16_t*>(take(rows * plan.blocks_per_row * 64 * sizeof(int16_t)));
        slots = take(rows * plan.row_stride);
        sizes = reinterpret_cast<int*>(take(rows * sizeof(int)));
        bytes = at;
    }
};

__global__ void __launch_bounds__(jpeg::kThreads) jpeg_transform_kernel(const unsigned char* __restrict__ pixels, int height, int width,
                                                                        int channels, int quality, Plan plan,
                                                                        int16_t* __restrict__ levels) {
    __shared__ jpeg::TransformShared sh;
    const int chunk = blockIdx.x % plan.chunks, row_of_all = blockIdx.x / plan.chunks;          // row_of_all = image * mcu_rows + row
    const int image = row_of_all / plan.mcu_rows, row = row_of_all - image * plan.mcu_rows;
    const int first = chunk * plan.chunk_mcus, left = plan.mcus_per_row - first;
    jpeg::transform_chunk(sh, pixels + (size_t)image * height * width * channels, height, width, channels, quality, row, first,
                          left < plan.chunk_mcus ? left : plan.chunk_mcus,
                          levels + ((size_t)row_of_all * plan.blocks_per_row + (size_t)first * (channels == 3 ? 6 : 1)) * 64);
}

__global__ void __launch_bounds__(jpeg::kThreads) jpeg_emit_kernel(const int16_t* __restrict__ levels, int colour, Plan plan,
                                                                   unsigned char* __restrict__ slots, int* __restrict__ sizes) {
    __shared__ jpeg::EmitShared sh;
    const int row = blockIdx.x % plan.mcu_rows;
    jpeg::emit_row(sh, levels + (size_t)blockIdx.x * plan.blocks_per_row * 64, plan.blocks_per_row, colour,
                   row == plan.mcu_rows - 1 ? -1 : row & 7, slots + (size_t)blockIdx.x * plan.row_stride, sizes + blockIdx.x);
}

__global__ void __launch_bounds__(jpeg::kThreads) jpeg_pack_kernel(const unsigned char* __restrict__ slots, const int* __restrict__ sizes,
                                                                   Plan plan, unsigned char* __restrict__ scans, size_t bound,
                                                                   long long* __restrict__ scan_bytes) {
    __shared__ jpeg::PackShared sh;
    const int image = blockIdx.x / plan.mcu_rows, row = blockIdx.x - image * plan.mcu_rows;
    jpeg::pack_row(sh, sizes + (size_t)image * plan.mcu_rows, row, plan.mcu_rows, slots + (size_t)blockIdx.x * plan.row_stride,
                   scans + (size_t)image * bound, scan_bytes + image);
}

}  // namespace

extern "C" size_t snerf_jpeg_scan_bound_bytes(int height, int width, int channels) {
    Plan plan;
    return plan_of(height, width, channels, &plan) ? bound_of(plan) : 0;
}

extern "C" size_t snerf_jpeg_scan_workspace_bytes(int images, int height, int width, int channels) {
    Plan plan;
    if (images < 1 || !plan_of(height, width, channels, &plan) || too_many(images, plan)) return 0;
    return Workspace(nullptr, images, plan).bytes;
}

extern "C" int snerf_jpeg_scan(const unsigned char* pixels, int images, int height, int width, int channels, int quality,
                               unsigned char* scans, long long* scan_bytes, void* workspace, snerf_stream_t stream) {
    Plan plan;
    SNERF_REQUIRE(channels == 1 || channels == 3, "jpeg_scan: channels %d, expected 1 or 3", channels);
    SNERF_REQUIRE(height >= 1 && height <= 65535 && width >= 1 && width <= 65535, "jpeg_scan: height %d, width %d outside 1..65535",
                  height, width);
    SNERF_REQUIRE(quality >= 1 && quality <= 100, "jpeg_scan: quality %d outside 1..100", quality);
    SNERF_REQUIRE(plan_of(height, width, channels, &plan), "jpeg_scan: %d x %d x %d", height, width, channels);
    SNERF_REQUIRE(images >= 0, "jpeg_scan: images %d", images);
    if (images == 0) return SNERF_OK;
    SNERF_REQUIRE(pixels && scans && scan_bytes && workspace, "jpeg_scan: NULL pointer");
    SNERF_REQUIRE(((unsigned long long)workspace & 15) == 0, "jpeg_scan: workspace must be 16-byte aligned");
    SNERF_REQUIRE(((unsigned long long)scan_bytes & 7) == 0, "jpeg_scan: scan_bytes must be 8-byte aligned");
    if (too_many(images, plan))
        return snerf::fail(SNERF_E_UNSUPPORTED, "jpeg_scan: %d images of %d MCU rows of %d chunks are 2^31 workgroups or more", images,
                           plan.mcu_rows, plan.chunks);
    const Workspace ws(workspace, images, plan);
    const size_t bound = bound_of(plan);
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(jpeg::kThreads);
    const unsigned rows = (unsigned)(images * plan.mcu_rows);
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3(rows * (unsigned)plan.chunks), block, 0, s, pixels, height, width, channels, quality,
                       plan, ws.levels);
    hipLaunchKernelGGL(jpeg_emit_kernel, dim3(rows), block, 0, s, ws.levels, (int)(channels == 3), plan, ws.slots, ws.sizes);
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3(rows), block, 0, s, ws.slots, ws.sizes, plan, scans, bound, scan_bytes);
    return snerf::check_launch("jpeg_scan");
}
