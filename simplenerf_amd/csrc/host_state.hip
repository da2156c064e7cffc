// The library's process-lifetime host state, each piece once (host_state.h holds the tables, free of HIP types):
//   per (device, stream)  StreamState: the enqueue lock, the side streams of a render, the layered path's inference scratch
//   per device            the fp16 range word, the CU count behind the persistent grids
//   per packed buffer     the operand formats its last pack call wrote
#include <unordered_map>
#include <vector>

#include "host_state.h"
#include "mlp_generic.h"
#include "snerf_common.h"

namespace snerf {

int current_device(int* device, bool clear_error) {
    if (hipGetDevice(device) == hipSuccess) return SNERF_OK;
    if (clear_error) (void)hipGetLastError();
    *device = -1;
    return SNERF_E_HIP;
}

// ---------------------------------------------------------------------------------------------------------------
// per (device, stream).  Everything but the mutex is read and written only by a call that holds it (a StreamLock).
struct ScratchBlock { float* base; size_t floats; };
struct StreamState : StreamStateBase {
    StreamState(int device_, hipStream_t stream_) : device(device_), stream(stream_) {}
    const int device;                     // -1: the lock of a call that had no current device
    const hipStream_t stream;
    SideStreams side;
    std::vector<ScratchBlock> scratch;    // generic_arena: never freed or moved, a larger request adds a block
};

namespace {
constexpr int kMaxSideSets = 64;
StreamTable<hipStream_t, StreamState, kMaxSideSets> g_streams;

StreamState* stream_state(hipStream_t stream) {
    int device = -1;
    (void)current_device(&device, true);      // (the call itself reports the missing device; it still enqueues nothing unlocked)
    return g_streams.find_or_create(device, stream);
}
}  // namespace

StreamLock::StreamLock(hipStream_t stream) : state_(stream_state(stream)) { state_->mutex.lock(); }
StreamLock::~StreamLock() { state_->mutex.unlock(); }

SideStreams* side_streams(const StreamLock& held) {
    StreamState* state = held.state();
    SideStreams& s = state->side;
    if (!s.ok) {
        if (state->device < 0 || !g_streams.grant(state)) return nullptr;
        bool good = hipEventCreateWithFlags(&s.fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < kSideStreams && good; ++i)
            good = hipStreamCreateWithFlags(&s.stream[i], hipStreamNonBlocking) == hipSuccess &&
                   hipEventCreateWithFlags(&s.join[i], hipEventDisableTiming) == hipSuccess;
        if (!good) {                 // (the caller falls back to one stream; nothing half-made stays behind)
            (void)hipGetLastError();
            if (s.fork) (void)hipEventDestroy(s.fork);
            for (int i = 0; i < kSideStreams; ++i) {
                if (s.join[i]) (void)hipEventDestroy(s.join[i]);
                if (s.stream[i]) (void)hipStreamDestroy(s.stream[i]);
            }
            s = SideStreams{};
            g_streams.give_back(state);
            return nullptr;
        }
        s.ok = true;
    }
    return &s;
}

// Scratch of the layered path's inference entry point (the ABI gives it no workspace argument): blocks of the caller's (device,
// stream), so that two layered-shape forwards on different streams of a device do not share an activation matrix (they
// used to); two threads on ONE stream take turns (the call holds the stream's StreamLock over all of its passes).  A block is NEVER
// freed or moved once handed out -- an in-flight kernel or a captured graph may hold its address; a larger request on the same
// stream allocates another block and the old one stays (sizes are bounded by kInferenceChunk rows, so a stream grows its block a
// handful of times at most).  Growing inside a graph capture is refused: the allocation would be a synchronous call the capture
// cannot contain.
int generic_arena(const StreamLock& held, size_t floats, float** out) {
    StreamState* state = held.state();
    if (state->device < 0) return fail(SNERF_E_HIP, "mlp_forward(layered): no current HIP device");
    for (const ScratchBlock& b : state->scratch)
        if (b.floats >= floats) {
            *out = b.base;
            return SNERF_OK;
        }
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(state->stream, &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone)
        return fail(SNERF_E_UNSUPPORTED, "mlp_forward(layered): the scratch block of this stream must grow to %zu MB, which a graph "
                                         "capture cannot contain -- run one call of this size on the stream before capturing",
                    floats * sizeof(float) >> 20);
    (void)hipGetLastError();
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, floats * sizeof(float));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(SNERF_E_HIP, "mlp_forward(layered): scratch of %zu MB: %s", floats * sizeof(float) >> 20, hipGetErrorString(e));
    }
    state->scratch.push_back({static_cast<float*>(p), floats});
    *out = static_cast<float*>(p);
    return SNERF_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// per device.  fp16 range flag: one int per device ordinal in pinned (host-coherent, device-mapped) memory.  Kernels store to it
// with a system-scope atomic when they met a non-finite fp16 operand; the host reads it without synchronising.
namespace {
std::mutex g_range_mutex;
int* g_range_table = nullptr;      // 64 ints
constexpr int kRangeDevices = 64;
DeviceValue g_compute_units;
}  // namespace

int* range_flag() {
    int device = 0;
    if (current_device(&device, false) != SNERF_OK || device < 0 || device >= kRangeDevices) {
        (void)fail(SNERF_E_HIP, "range flag: no current HIP device (or ordinal >= %d)", kRangeDevices);
        return nullptr;
    }
    std::lock_guard<std::mutex> lock(g_range_mutex);
    if (!g_range_table) {
        void* p = nullptr;
        const hipError_t e = hipHostMalloc(&p, kRangeDevices * sizeof(int), hipHostMallocPortable | hipHostMallocMapped);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)fail(SNERF_E_HIP, "range flag: hipHostMalloc: %s (the first fp16-mode call of a process must not be inside "
                                    "a graph capture)", hipGetErrorString(e));
            return nullptr;
        }
        g_range_table = static_cast<int*>(p);
        for (int i = 0; i < kRangeDevices; ++i) g_range_table[i] = 0;
    }
    return g_range_table + device;
}

int report_range(const char* what) {
    int* flag = range_flag();
    if (!flag) return SNERF_E_HIP;
    const int bits = __atomic_exchange_n(flag, 0, __ATOMIC_ACQ_REL);
    if (bits == 0) return SNERF_OK;
    return fail(SNERF_E_RANGE, "%s: an earlier fp16-mode launch on this device met %s%s%s outside the fp16 range (|v| > 65504): "
                               "its results are invalid -- use hip_precision 'fp32' for this model", what,
                (bits & kRangeActivation) ? "a hidden activation or encoded input" : "", (bits & kRangeActivation) && (bits & kRangeWeight) ? " and " : "",
                (bits & kRangeWeight) ? "a weight" : "");
}

unsigned persistent_workgroups() {
    int device = -1, cus = 256;
    if (current_device(&device, false) == SNERF_OK) {
        const int known = g_compute_units.get(device, [device]() {
            int value = 0;
            return hipDeviceGetAttribute(&value, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess ? value : 0;
        });
        if (known > 0) cus = known;
    }
    (void)hipGetLastError();
    const unsigned count = (unsigned)(2 * cus) & ~7u;
    return count ? count : 8u;
}

// ---------------------------------------------------------------------------------------------------------------
// packed-format registry (snerf_common.h)
namespace {
std::mutex g_formats_mutex;
std::unordered_map<const float*, unsigned> g_formats;
constexpr size_t kFormatsCapacity = 1 << 16;     // distinct packed buffers remembered; beyond it the table starts over

const char* formats_text(unsigned formats, char* buffer, size_t size) {
    snprintf(buffer, size, "%s%s%s%s%s", (formats & kPackFp32) ? "fp32 " : "", (formats & kPackF16) ? "f16-training " : "",
             (formats & kPackF16Eval) ? "f16-rendering " : "", (formats & kPackBf16) ? "bf16-training " : "",
             (formats & kPackBf16Eval) ? "bf16-rendering " : "");
    return buffer;
}
}  // namespace

void packed_formats_record(const float* packed, unsigned formats) {
    std::lock_guard<std::mutex> lock(g_formats_mutex);
    if (g_formats.size() >= kFormatsCapacity) g_formats.clear();
    g_formats[packed] = formats;
}

int packed_formats_require(const float* packed, unsigned needed, const char* what) {
    unsigned have;
    {
        std::lock_guard<std::mutex> lock(g_formats_mutex);
        auto it = g_formats.find(packed);
        if (it == g_formats.end()) return SNERF_OK;       // never packed through this library instance: cannot tell
        have = it->second;
    }
    if ((have & needed) == needed) return SNERF_OK;
    char a[96], b[96];
    return fail(SNERF_E_INVALID, "%s: this packed buffer holds the operand formats [ %s] (its last snerf_mlp_pack_for), the call reads "
                                 "[ %s]: the missing streams are zero-filled -- pack with snerf_mlp_pack, or snerf_mlp_pack_for the "
                                 "precision and mode it is used at", what, formats_text(have, a, sizeof a),
                formats_text(needed, b, sizeof b));
}

unsigned packed_formats_needed(int precision, bool training) {
    switch (precision) {
        case SNERF_PRECISION_FP32: return kPackFp32;
        case SNERF_PRECISION_F16X3: case SNERF_PRECISION_F16: case SNERF_PRECISION_F16S8:
            return kPackF16 | (training ? 0u : kPackF16Eval);
        case SNERF_PRECISION_BF16: case SNERF_PRECISION_BF16S8: return kPackBf16 | (training ? 0u : kPackBf16Eval);
        default: return 0u;
    }
}

}  // namespace snerf

extern "C" int snerf_range_status(int clear) {
    int* flag = snerf::range_flag();
    if (!flag) return SNERF_E_HIP;
    return clear ? __atomic_exchange_n(flag, 0, __ATOMIC_ACQ_REL) : __atomic_load_n(flag, __ATOMIC_ACQUIRE);
}
