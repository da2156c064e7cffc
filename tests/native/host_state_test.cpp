// simplenerf_amd/csrc/host_state.h on the host, with fake stream handles (no GPU; built once with ThreadSanitizer and once with
// AddressSanitizer + UBSan by tests/test_host_state_host.py): one State per (device, stream) behind a pointer that never moves, its
// recursive mutex as the only guard of what the State holds, the cap on granted States, and the per-device cached value.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../simplenerf_amd/csrc/host_state.h"

using FakeStream = const char*;      // compared and ordered like a handle, never dereferenced

struct State : snerf::StreamStateBase {
    State(int device_, FakeStream stream_) : device(device_), stream(stream_) {}
    const int device;
    const FakeStream stream;
    int plain = 0;                   // guarded by `mutex` alone
};
using Table = snerf::StreamTable<FakeStream, State, 64>;

static int fails = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                                    \
        }                                                               \
    } while (0)

static char handles[1 << 16];        // addresses to serve as streams
static FakeStream stream_of(int i) { return handles + i; }

// 8 threads x 64 keys (4 devices x 16 streams) x 4000 find-or-create calls, every 16th call inserting a fresh key of the thread's own:
// every thread sees the same pointer per key, and a pointer taken first still addresses the same object after >= 1 000 more inserts
static void check_stable_pointers() {
    Table table;
    constexpr int kThreads = 8, kKeys = 64, kCalls = 4000;
    State* first[kKeys];
    for (int k = 0; k < kKeys; ++k) first[k] = table.find_or_create(k / 16, stream_of(k % 16));
    std::atomic<int> wrong{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < kThreads; ++t)
        pool.emplace_back([&, t]() {
            for (int i = 0; i < kCalls; ++i) {
                const int k = (i * 7 + t) % kKeys;
                if (table.find_or_create(k / 16, stream_of(k % 16)) != first[k]) wrong.fetch_add(1);
                if (i % 16 == 0) {
                    State* fresh = table.find_or_create(100 + t, stream_of(1000 + i));
                    if (fresh->device != 100 + t || fresh->stream != stream_of(1000 + i)) wrong.fetch_add(1);
                }
            }
        });
    for (auto& th : pool) th.join();
    CHECK(wrong.load() == 0);                        // (8 x 250 = 2 000 fresh keys went in meanwhile)
    for (int i = 0; i < 1000; ++i) (void)table.find_or_create(7, stream_of(20000 + i));
    for (int k = 0; k < kKeys; ++k) {
        CHECK(table.find_or_create(k / 16, stream_of(k % 16)) == first[k]);
        CHECK(first[k]->device == k / 16 && first[k]->stream == stream_of(k % 16) && first[k]->plain == 0);
    }
    // the key is the pair: one stream on two devices, two streams on one device, the no-device ordinal
    CHECK(table.find_or_create(0, stream_of(0)) != table.find_or_create(1, stream_of(0)));
    CHECK(table.find_or_create(0, stream_of(0)) != table.find_or_create(0, stream_of(1)));
    CHECK(table.find_or_create(-1, stream_of(0)) != table.find_or_create(0, stream_of(0)) && table.find_or_create(-1, stream_of(0))->device == -1);
    CHECK(table.find_or_create(0, nullptr) == table.find_or_create(0, nullptr));
}

// the enqueue lock is recursive (a render holds it while the MLP entry points it calls take it again), and it is the ONLY guard of the
// State's other members: two threads, 100 000 increments of a plain int each, only under that key's lock
static void check_lock() {
    Table table;
    State* s = table.find_or_create(0, stream_of(3));
    s->mutex.lock();
    s->mutex.lock();
    s->plain = 5;
    s->mutex.unlock();
    s->mutex.unlock();
    CHECK(s->mutex.try_lock());
    s->mutex.unlock();
    s->plain = 0;
    std::vector<std::thread> pool;
    for (int t = 0; t < 2; ++t)
        pool.emplace_back([&]() {
            for (int i = 0; i < 100000; ++i) {
                State* mine = table.find_or_create(0, stream_of(3));
                std::lock_guard<std::recursive_mutex> outer(mine->mutex);
                std::lock_guard<std::recursive_mutex> inner(mine->mutex);
                ++mine->plain;
            }
        });
    for (auto& th : pool) th.join();
    CHECK(s->plain == 200000);
}

static void check_cap() {
    Table table;
    std::vector<State*> states;
    for (int i = 0; i < 70; ++i) states.push_back(table.find_or_create(i % 2, stream_of(i)));
    for (int i = 0; i < 64; ++i) CHECK(table.grant(states[i]));
    CHECK(!table.grant(states[64]) && !table.grant(states[65]));        // the 65th distinct key that asks
    CHECK(!table.grant(states[64]));                                    // ... and again
    for (int i = 0; i < 64; ++i) CHECK(table.grant(states[i]));         // a granted key asking again
    table.give_back(states[10]);                                        // its set-up failed: the slot is free again
    CHECK(table.grant(states[64]) && !table.grant(states[10]) && !table.grant(states[65]));
    table.give_back(states[65]);                                        // never granted: nothing to give back
    CHECK(!table.grant(states[66]));
    table.give_back(states[64]);
    CHECK(table.grant(states[10]) && !table.grant(states[64]));
    // racing askers: exactly the cap is granted
    Table racing;
    std::atomic<int> granted{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < 8; ++t)
        pool.emplace_back([&, t]() {
            for (int i = 0; i < 32; ++i) {
                State* s = racing.find_or_create(t, stream_of(i));
                std::lock_guard<std::recursive_mutex> lock(s->mutex);
                if (racing.grant(s)) granted.fetch_add(1);
            }
        });
    for (auto& th : pool) th.join();
    CHECK(granted.load() == 64);
}

static void check_device_value() {
    snerf::DeviceValue cache;
    int calls[300] = {};
    auto compute = [&](int dev, int result) { return [&calls, dev, result]() { ++calls[dev]; return result; }; };
    CHECK(cache.get(0, compute(0, 256)) == 256 && cache.get(0, compute(0, 999)) == 256 && calls[0] == 1);
    CHECK(cache.get(1, compute(1, 304)) == 304 && cache.get(1, compute(1, 999)) == 304 && cache.get(0, compute(0, 999)) == 256);
    CHECK(calls[0] == 1 && calls[1] == 1);
    // a failure (<= 0) is passed on and not remembered
    CHECK(cache.get(7, compute(7, 0)) == 0 && cache.get(7, compute(7, -3)) == -3 && cache.get(7, compute(7, 64)) == 64);
    CHECK(cache.get(7, compute(7, 999)) == 64 && calls[7] == 3);
    // the last ordinal of the table, and ordinals beyond it: computed every time
    CHECK(cache.get(255, compute(255, 8)) == 8 && cache.get(255, compute(255, 9)) == 8 && calls[255] == 1);
    CHECK(cache.get(256, compute(256, 8)) == 8 && cache.get(256, compute(256, 9)) == 9 && calls[256] == 2);
    CHECK(cache.get(-1, compute(299, 8)) == 8 && cache.get(-1, compute(299, 8)) == 8 && calls[299] == 2);
    // racing threads: each may compute until one success is published, nobody afterwards
    snerf::DeviceValue shared;
    std::atomic<int> ran[8] = {};
    std::atomic<int> wrong{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < 32; ++t)
        pool.emplace_back([&, t]() {
            for (int i = 0; i < 1000; ++i)
                if (shared.get(t % 8, [&]() { ran[t % 8].fetch_add(1); return 100 + t % 8; }) != 100 + t % 8) wrong.fetch_add(1);
        });
    for (auto& th : pool) th.join();
    CHECK(wrong.load() == 0);
    for (int d = 0; d < 8; ++d) {
        const int before = ran[d].load();
        CHECK(before >= 1 && before <= 4);           // (four threads per ordinal)
        CHECK(shared.get(d, [&]() { ran[d].fetch_add(1); return 1; }) == 100 + d && ran[d].load() == before);
    }
}

int main() {
    check_stable_pointers();
    check_lock();
    check_cap();
    check_device_value();
    if (fails == 0) std::printf("host_state_test: OK\n");
    return fails == 0 ? 0 : 1;
}
