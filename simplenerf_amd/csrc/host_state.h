// What the library remembers on the host for the life of the process, keyed by (device, stream) or by device ordinal: the tables
// themselves, free of HIP types so that a plain C++ program can drive them with fake handles (tests/native/host_state_test.cpp,
// under ThreadSanitizer and AddressSanitizer).  host_state.hip instantiates them with hipStream_t and owns what hangs off them.
//
// StreamTable: find-or-create of ONE State per (device, stream).  A State lives behind a pointer that never moves and is never freed
// (a thread may hold one State's mutex while another thread creates the next; a captured graph may hold what the State owns).  The
// lookup runs under the table's one mutex; everything else in a State is guarded by the State's OWN recursive mutex -- the stream's
// enqueue lock -- which a caller holds from its first launch to its last.  That is why a State's members need no locks of their own.
//
// DeviceValue: a positive int cached per device ordinal (DeviceOnce's contract: racing threads may both compute it, a failure is
// not remembered, ordinals beyond the table are computed every time).
#pragma once
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <utility>

namespace snerf {

// What every State of a StreamTable begins with.  `granted` belongs to the table (StreamTable::grant).
struct StreamStateBase {
    std::recursive_mutex mutex;      // the stream's enqueue lock
    bool granted = false;
};

// State: derived from StreamStateBase, constructible from (int device, Stream stream).  Cap: how many States may hold a grant.
template <class Stream, class State, int Cap>
class StreamTable {
public:
    State* find_or_create(int device, Stream stream) {
        std::lock_guard<std::mutex> lock(mutex_);
        std::unique_ptr<State>& state = states_[{device, stream}];
        if (!state) state.reset(new State(device, stream));
        return state.get();
    }

    // A capped resource (the side streams of a render): the first Cap States that ask are granted, the rest refused; a granted State
    // asking again is still granted; a State whose set-up failed gives its slot back and may ask again.
    bool grant(State* state) {
        std::lock_guard<std::mutex> lock(mutex_);
        StreamStateBase* base = state;
        if (!base->granted && granted_ < Cap) { base->granted = true; ++granted_; }
        return base->granted;
    }
    void give_back(State* state) {
        std::lock_guard<std::mutex> lock(mutex_);
        StreamStateBase* base = state;
        if (base->granted) { base->granted = false; --granted_; }
    }

private:
    std::mutex mutex_;
    std::map<std::pair<int, Stream>, std::unique_ptr<State>> states_;
    int granted_ = 0;
};

struct DeviceValue {
    static constexpr int kDevices = 256;
    std::atomic<int> value[kDevices] = {};      // 0: not known yet

    // The cached value of `device`, else what `compute()` returns -- remembered when it is positive (<= 0: a failure, passed on).
    template <class Compute>
    int get(int device, Compute&& compute) {
        const bool cached = device >= 0 && device < kDevices;
        if (cached) {
            const int known = value[device].load(std::memory_order_acquire);
            if (known > 0) return known;
        }
        const int fresh = compute();
        if (cached && fresh > 0) value[device].store(fresh, std::memory_order_release);
        return fresh;
    }
};

}  // namespace snerf
