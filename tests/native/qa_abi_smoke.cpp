// The depth metrics' rank statistics and a stable key order from the C ABI alone: plain HIP runtime + include/simplenerf_hip.h, linked
// against libsimplenerf_hip.so, no torch in the process.  A 37 x 53 depth pair and a mask with many ties are built from integer
// expressions; the library sorts them (snerf_sort_f32), selects the masked pixels (snerf_compact_f32_pair) and reduces them
// (snerf_depth_error_sums, snerf_rank_correlation_sums); the median, DepthSROCC and MaskedDepthSROCC are compared with std::stable_sort
// and straightforward tie-averaged ranks computed here, and the order of snerf_sort_keys_with_order with std::stable_sort's.
// Built and run by tests/test_gpu_qa_native.py.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "simplenerf_hip.h"

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

template <typename T>
static T* dev(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) std::abort();
    return static_cast<T*>(p);
}
template <typename T>
static T* upload(const std::vector<T>& h) {
    T* d = dev<T>(h.size());
    if (hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) std::abort();
    return d;
}
template <typename T>
static std::vector<T> host(const T* d, size_t n) {
    std::vector<T> h(n);
    if (n && hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) std::abort();
    return h;
}

// Centred tie-averaged ranks: a value's rank is the mean of the 1-based sorted positions of its run, minus (n + 1) / 2.
static std::vector<double> ranks(const std::vector<float>& v) {
    const size_t n = v.size();
    std::vector<size_t> index(n);
    std::iota(index.begin(), index.end(), size_t(0));
    std::stable_sort(index.begin(), index.end(), [&](size_t a, size_t b) { return v[a] < v[b]; });
    std::vector<double> r(n);
    for (size_t first = 0; first < n;) {
        size_t last = first;
        while (last + 1 < n && v[index[last + 1]] == v[index[first]]) ++last;
        const double mean = 0.5 * double(first + 1 + last + 1) - 0.5 * double(n + 1);
        for (size_t k = first; k <= last; ++k) r[index[k]] = mean;
        first = last + 1;
    }
    return r;
}

static double spearman(const std::vector<float>& x, const std::vector<float>& y) {
    const std::vector<double> rx = ranks(x), ry = ranks(y);
    double xy = 0, xx = 0, yy = 0;
    for (size_t i = 0; i < x.size(); ++i) {
        xy += rx[i] * ry[i];
        xx += rx[i] * rx[i];
        yy += ry[i] * ry[i];
    }
    return xy / std::sqrt(xx) / std::sqrt(yy);
}

int main() {
    CHECK(snerf_abi_version() == SNERF_ABI_VERSION);
    const int h = 37, w = 53;
    const long long n = (long long)h * w;
    std::vector<float> gt(n), eval(n);
    std::vector<unsigned char> mask(n);
    for (long long i = 0; i < n; ++i) {
        const long long y = i / w, x = i % w;
        gt[i] = 1.0f + 0.25f * float((3 * y + 2 * x) % 29);                    // 29 distinct values: long runs of ties
        eval[i] = 0.75f + 0.125f * float((6 * y + 4 * x + (i * i) % 7) % 61);  // follows gt, with its own ties
        mask[i] = (unsigned char)(((i * i + 3 * i) % 5 < 3) ? ((i & 1) ? 255 : 1) : 0);
    }
    float *d_gt = upload(gt), *d_eval = upload(eval), *d_sorted_gt = dev<float>(n), *d_sorted_eval = dev<float>(n);
    unsigned char* d_mask = upload(mask);
    void* sort_ws = dev<char>((size_t)snerf_sort_workspace_bytes(n, 32));
    void* metric_ws = dev<char>((size_t)snerf_metrics_workspace_bytes(h, w));
    void* compact_ws = dev<char>((size_t)snerf_compact_workspace_bytes(n));
    double *d_error = dev<double>(4), *d_rank = dev<double>(3), *d_masked_rank = dev<double>(3);
    CHECK(snerf_sort_workspace_bytes(n, 32) > 0 && snerf_compact_workspace_bytes(n) > 0);

    // the median and DepthSROCC
    SNERF_OK_(snerf_sort_f32(d_gt, n, d_sorted_gt, sort_ws, nullptr));
    SNERF_OK_(snerf_sort_f32(d_eval, n, d_sorted_eval, sort_ws, nullptr));
    SNERF_OK_(snerf_depth_error_sums(d_gt, d_eval, 1.0, 1.0, nullptr, n, d_sorted_gt, d_error, metric_ws, nullptr));
    SNERF_OK_(snerf_rank_correlation_sums(d_gt, d_eval, d_sorted_gt, d_sorted_eval, n, d_rank, metric_ws, nullptr));
    // the masked pixels, in order, and their count
    float *d_gt_kept = dev<float>(n), *d_eval_kept = dev<float>(n);
    long long* d_kept = dev<long long>(1);
    SNERF_OK_(snerf_compact_f32_pair(d_gt, d_eval, d_mask, n, d_gt_kept, d_eval_kept, d_kept, compact_ws, nullptr));
    HIP_OK(hipDeviceSynchronize());
    const long long kept = host(d_kept, 1)[0];
    std::vector<float> gt_kept, eval_kept;
    for (long long i = 0; i < n; ++i)
        if (mask[i]) {
            gt_kept.push_back(gt[i]);
            eval_kept.push_back(eval[i]);
        }
    CHECK(kept == (long long)gt_kept.size() && kept > n / 4 && kept < n);
    CHECK(host(d_gt_kept, kept) == gt_kept && host(d_eval_kept, kept) == eval_kept);
    // MaskedDepthSROCC
    float *d_sorted_gt_kept = dev<float>(kept), *d_sorted_eval_kept = dev<float>(kept);
    SNERF_OK_(snerf_sort_f32(d_gt_kept, kept, d_sorted_gt_kept, sort_ws, nullptr));
    SNERF_OK_(snerf_sort_f32(d_eval_kept, kept, d_sorted_eval_kept, sort_ws, nullptr));
    SNERF_OK_(snerf_rank_correlation_sums(d_gt_kept, d_eval_kept, d_sorted_gt_kept, d_sorted_eval_kept, kept, d_masked_rank, metric_ws, nullptr));
    HIP_OK(hipDeviceSynchronize());

    std::vector<float> want_sorted = gt;
    std::stable_sort(want_sorted.begin(), want_sorted.end());
    CHECK(host(d_sorted_gt, n) == want_sorted);
    const std::vector<double> error = host(d_error, 4), rank = host(d_rank, 3), masked_rank = host(d_masked_rank, 3);
    const double median = error[3], want_median = (n & 1) ? double(want_sorted[n / 2]) : 0.5 * (double(want_sorted[n / 2 - 1]) + double(want_sorted[n / 2]));
    const double srocc = rank[0] / std::sqrt(rank[1]) / std::sqrt(rank[2]), want_srocc = spearman(gt, eval);
    const double masked_srocc = masked_rank[0] / std::sqrt(masked_rank[1]) / std::sqrt(masked_rank[2]), want_masked_srocc = spearman(gt_kept, eval_kept);
    std::printf("median %.17g (%.17g)  DepthSROCC %.17g (%.17g)  MaskedDepthSROCC %.17g (%.17g)  kept %lld of %lld\n", median, want_median,
                srocc, want_srocc, masked_srocc, want_masked_srocc, kept, n);
    CHECK(median == want_median);
    CHECK(std::fabs(want_srocc) > 0.05 && std::fabs(want_srocc) < 0.999);      // neither uncorrelated nor a copy
    CHECK(std::fabs(srocc - want_srocc) <= 1e-10);
    CHECK(std::fabs(masked_srocc - want_masked_srocc) <= 1e-10);
    CHECK(error[2] == double(n));

    // the stable order of a small key array: 97 distinct keys over three tiles and a ragged tail
    const long long m = 3 * 2048 + 17;
    const int key_bits = 7;
    std::vector<int> keys(m);
    for (long long i = 0; i < m; ++i) keys[i] = int((i * i * 31 + i * 7) % 97);
    int *d_keys = upload(keys), *d_sorted_keys = dev<int>(m);
    long long* d_order = dev<long long>(m);
    void* key_ws = dev<char>((size_t)snerf_sort_workspace_bytes(m, key_bits));
    SNERF_OK_(snerf_sort_keys_with_order(d_keys, m, key_bits, d_sorted_keys, d_order, key_ws, nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<long long> want_order(m);
    std::iota(want_order.begin(), want_order.end(), 0LL);
    std::stable_sort(want_order.begin(), want_order.end(), [&](long long a, long long b) { return keys[a] < keys[b]; });
    const std::vector<long long> order = host(d_order, m);
    const std::vector<int> sorted_keys = host(d_sorted_keys, m);
    CHECK(order == want_order);
    for (long long j = 0; j < m; ++j) CHECK(sorted_keys[j] == keys[want_order[j]]);
    CHECK(host(d_keys, m) == keys && host(d_gt, n) == gt);                     // inputs are not written

    // refusals carry the argument's name
    CHECK(snerf_sort_f32(nullptr, n, d_sorted_gt, sort_ws, nullptr) == SNERF_E_INVALID);
    CHECK(snerf_sort_keys_with_order(d_keys, m, 33, d_sorted_keys, d_order, key_ws, nullptr) == SNERF_E_INVALID);
    std::printf("qa_abi_smoke: OK\n");
    return 0;
}
