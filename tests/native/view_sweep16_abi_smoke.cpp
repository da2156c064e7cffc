// The 16-bit view sweep from the C ABI alone: plain HIP runtime + include/simplenerf_hip.h + csrc/simplenerf_sweep16.h, linked
// against libsimplenerf_hip.so, no PyTorch in the process.  The scene of view_sweep_abi_smoke.cpp (a seeded 4 x 128 / 64 MLP on the
// 35 rays of a 5 x 7 frame with 20 samples each: rays straddle the 32-sample blocks, the last block is partial; white background),
// once at SNERF_PRECISION_F16 and once at SNERF_PRECISION_BF16:
//     snerf_mlp_forward_train -> snerf_composite -> snerf_view_sweep_half over three sets of view directions
// and every view against snerf_mlp_forward + snerf_composite at the same precision with that view's directions.  The tolerance is
// computed here: the formula of simplenerf_sweep16.h restated on the host in float and in double on the feature pieces the device
// saved -- decoded by that header's layout text -- and on weights and encodings rounded as it says, their largest difference
// times 4 (the device sums each dot product in another order).  Built and run by tests/test_gpu_view_sweep16_native.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simplenerf_hip.h"
#include "simplenerf_sweep16.h"

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
static std::vector<T> host(const T* d, size_t n) {
    std::vector<T> h(n);
    if (hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) std::abort();
    return h;
}

constexpr int kDepth = 4, kWidth = 128, kViewsWidth = 64, kDegree = 4, kViewsIn = kWidth + 3 + 6 * kDegree;

// the value of a 16-bit pattern, and r(): fp32 -> the format, round to nearest even, -> fp32 (finite inputs of ordinary size)
static float widen(uint16_t bits, bool bf) {
    if (bf) {
        const uint32_t word = (uint32_t)bits << 16;
        float v;
        std::memcpy(&v, &word, 4);
        return v;
    }
    _Float16 half;
    std::memcpy(&half, &bits, 2);
    return (float)half;
}
static float rounded(float v, bool bf) {
    if (!bf) return (float)(_Float16)v;
    uint32_t word;
    std::memcpy(&word, &v, 4);
    word += 0x7fffu + ((word >> 16) & 1u);
    return widen((uint16_t)(word >> 16), true);
}

// out[v][ray][c] of simplenerf_sweep16.h on operands that are already rounded, every operation in T
template <typename T>
static std::vector<T> restate(const std::vector<float>& wv, const std::vector<float>& bv, const std::vector<float>& wo,
                              const std::vector<float>& bo, const std::vector<float>& feature, const std::vector<float>& weights,
                              const std::vector<float>& acc, const std::vector<float>& dirs, long long n, int s, int views, bool bf) {
    std::vector<T> out((size_t)views * n * 3), g((size_t)n * s * kViewsWidth);
    for (long long i = 0; i < n * s; ++i)
        for (int j = 0; j < kViewsWidth; ++j) {
            T sum = 0;
            for (int k = 0; k < kWidth; ++k) sum += (T)wv[(size_t)j * kViewsIn + k] * (T)feature[(size_t)i * kWidth + k];
            g[(size_t)i * kViewsWidth + j] = sum;
        }
    for (int v = 0; v < views; ++v)
        for (long long r = 0; r < n; ++r) {
            T pe[3 + 6 * kDegree], u[kViewsWidth];
            for (int d = 0; d < 3; ++d) {
                const float x = dirs[((size_t)v * n + r) * 3 + d];
                pe[d] = (T)rounded(x, bf);
                for (int k = 0; k < kDegree; ++k) {      // the encoding is an fp32 quantity before it is rounded, in either restatement
                    pe[3 + 6 * k + d] = (T)rounded((float)std::sin((double)x * (1 << k)), bf);
                    pe[6 + 6 * k + d] = (T)rounded((float)std::cos((double)x * (1 << k)), bf);
                }
            }
            for (int j = 0; j < kViewsWidth; ++j) {
                T sum = (T)bv[j];
                for (int e = 0; e < 3 + 6 * kDegree; ++e) sum += (T)wv[(size_t)j * kViewsIn + kWidth + e] * pe[e];
                u[j] = sum;
            }
            T colour[3] = {0, 0, 0};
            for (int k = 0; k < s; ++k) {
                const size_t i = (size_t)r * s + k;
                for (int c = 0; c < 3; ++c) {
                    T pre = (T)bo[c];
                    for (int j = 0; j < kViewsWidth; ++j) {
                        const T hidden = g[i * kViewsWidth + j] + u[j];
                        pre += (T)wo[(size_t)c * kViewsWidth + j] * (hidden > 0 ? hidden : (T)0);
                    }
                    colour[c] += (T)weights[i] * ((T)1 / ((T)1 + std::exp(-pre)));
                }
            }
            for (int c = 0; c < 3; ++c) out[((size_t)v * n + r) * 3 + c] = colour[c] + ((T)1 - (T)acc[r]);
        }
    return out;
}

int main() {
    CHECK(snerf_abi_version() == SNERF_ABI_VERSION);
    const int h = 5, w = 7, S = 20, V = 3;
    const long long n = (long long)h * w;
    const float intrinsic[9] = {9.f, 0.f, 3.5f, 0.f, 9.f, 2.5f, 0.f, 0.f, 1.f};
    const float pose[16] = {1, 0, 0, 0.1f, 0, 1, 0, -0.2f, 0, 0, 1, 0.3f, 0, 0, 0, 1};
    float *rays_o = dev<float>(3 * n), *rays_d = dev<float>(3 * n), *own_dirs = dev<float>(3 * n), *view_dirs = dev<float>(3 * n * V),
          *scratch_o = dev<float>(3 * n), *scratch_d = dev<float>(3 * n);
    SNERF_OK_(snerf_generate_rays(h, w, intrinsic, pose, 0.f, 0, 1.f, 0, n, rays_o, rays_d, own_dirs, nullptr, nullptr, nullptr));
    for (int v = 0; v < V; ++v) {      // three other cameras: rotated about y, shifted, another focal length
        const float a = 0.3f * (v + 1), c = std::cos(a), s = std::sin(a);
        const float view_pose[16] = {c, 0, s, 0.5f * v, 0, 1, 0, 0.1f, -s, 0, c, -0.2f * v, 0, 0, 0, 1};
        const float view_intrinsic[9] = {7.f + v, 0.f, 3.5f, 0.f, 8.f, 2.5f, 0.f, 0.f, 1.f};
        SNERF_OK_(snerf_generate_rays(h, w, view_intrinsic, view_pose, 0.f, 0, 1.f, 0, n, scratch_o, scratch_d, view_dirs + 3 * n * v,
                                      nullptr, nullptr, nullptr));
    }
    float *near = dev<float>(n), *far = dev<float>(n), *depths = dev<float>(n * S);
    std::vector<float> twos(n, 2.f), sixes(n, 6.f);
    HIP_OK(hipMemcpy(near, twos.data(), n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(far, sixes.data(), n * 4, hipMemcpyHostToDevice));
    SNERF_OK_(snerf_coarse_depths(near, far, n, S, 0, nullptr, depths, nullptr));

    snerf_mlp_desc desc = {kDepth, kWidth, 1, kViewsWidth, 10, kDegree, -1, 1, 1};
    const int np = snerf_mlp_num_params(&desc);
    CHECK(np == 16);
    const int shape[16][2] = {{128, 63}, {128, 1}, {128, 128}, {128, 1}, {128, 128}, {128, 1}, {128, 128}, {128, 1},
                              {1, 128},  {1, 1},   {128, 128}, {128, 1}, {64, kViewsIn}, {64, 1},  {3, 64},    {3, 1}};
    std::vector<float*> params(np);
    std::vector<std::vector<float>> host_params(np);
    unsigned state = 2024u;
    for (int i = 0; i < np; ++i) {
        const size_t count = (size_t)shape[i][0] * shape[i][1];
        host_params[i].resize(count);
        float scale = (i & 1) ? 0.05f : 1.5f / std::sqrt((float)shape[i][1]);
        if (i == 8) scale *= 20.f;          // the density head: not a transparent field
        for (float& v : host_params[i]) {
            state = state * 1664525u + 1013904223u;
            v = scale * ((float)(state >> 8) / 8388608.f - 1.f);
        }
        if (i == 9) host_params[i][0] = 0.4f;
        params[i] = dev<float>(count);
        HIP_OK(hipMemcpy(params[i], host_params[i].data(), count * 4, hipMemcpyHostToDevice));
    }
    float* packed = dev<float>(snerf_mlp_packed_floats(&desc));
    SNERF_OK_(snerf_mlp_pack(&desc, params.data(), np, packed, nullptr));

    const size_t saved_floats = snerf_mlp_saved_floats(&desc, n, S), read_floats = snerf_view_sweep_half_acts_floats(&desc, n, S);
    CHECK(read_floats > 0 && read_floats <= saved_floats);
    const size_t work_floats = snerf_view_sweep_half_workspace_floats(&desc, n, S, V);
    CHECK(work_floats > 0 && snerf_view_sweep_half_workspace_floats(&desc, n, S, V + 1) >= work_floats);
    float *sigma = dev<float>(n * S), *rgb = dev<float>(3 * n * S), *saved = dev<float>(saved_floats);
    float *out_rgb = dev<float>(3 * n), *acc = dev<float>(n), *weights = dev<float>(n * S), *depth = dev<float>(n), *depth_var = dev<float>(n);
    float *work = dev<float>(work_floats), *swept = dev<float>(3 * n * V), *again = dev<float>(3 * n * V), *ordinary = dev<float>(3 * n * V);
    // rows of 32 x 16 bit (simplenerf_sweep16.h)
    const int act_feature = 96 + kDepth * kWidth, mask_tiles = kDepth * (kWidth / 32) + kViewsWidth / 32;
    const int block_rows = 96 + (kDepth + 1) * kWidth + kViewsWidth + 4 * ((mask_tiles + 1) / 2);

    for (int mode = 0; mode < 2; ++mode) {
        const bool bf = mode == 1;
        const int precision = bf ? SNERF_PRECISION_BF16 : SNERF_PRECISION_F16;
        const char* name = bf ? "bf16" : "f16";
        // the chain: storing forward -> compositing -> sweep
        SNERF_OK_(snerf_mlp_forward_train(&desc, packed, rays_o, rays_d, own_dirs, depths, n, S, nullptr, sigma, rgb, saved, precision, nullptr));
        SNERF_OK_(snerf_composite(sigma, rgb, depths, rays_d, nullptr, nullptr, n, S, 0, 1, out_rgb, acc, nullptr, nullptr, weights, depth,
                                  depth_var, nullptr, nullptr, nullptr));
        SNERF_OK_(snerf_view_sweep_half(&desc, params.data(), np, saved, weights, acc, view_dirs, n, S, V, 1, precision, swept, work, nullptr));
        SNERF_OK_(snerf_view_sweep_half(&desc, params.data(), np, saved, weights, acc, view_dirs, n, S, V, 1, precision, again, work, nullptr));
        // the same views one by one through the ordinary sequence
        for (int v = 0; v < V; ++v) {
            SNERF_OK_(snerf_mlp_forward(&desc, packed, rays_o, rays_d, view_dirs + 3 * n * v, depths, n, S, nullptr, sigma, rgb, precision, nullptr));
            SNERF_OK_(snerf_composite(sigma, rgb, depths, rays_d, nullptr, nullptr, n, S, 0, 1, ordinary + 3 * n * v, acc, nullptr, nullptr,
                                      nullptr, depth, depth_var, nullptr, nullptr, nullptr));
        }
        HIP_OK(hipDeviceSynchronize());

        // the device's own operands: the pieces by the header's text, the weights rounded as it says
        auto pieces = host(reinterpret_cast<const uint16_t*>(saved), 2 * read_floats);
        std::vector<float> feature((size_t)n * S * kWidth);
        for (long long i = 0; i < n * S; ++i) {
            const size_t first = ((size_t)(i / 32) * block_rows + act_feature) * 32;
            const int j = (int)(i % 32);
            for (int k = 0; k < kWidth / 16; ++k)
                for (int half = 0; half < 2; ++half)
                    for (int e = 0; e < 8; ++e)
                        feature[(size_t)i * kWidth + 16 * k + 8 * (e >> 2) + 4 * half + (e & 3)] =
                            widen(pieces[first + (size_t)k * 512 + (2 * j + half) * 8 + e], bf);
        }
        std::vector<float> wv = host_params[12];
        for (float& v : wv) v = rounded(v, bf);
        auto hw = host(weights, n * S), ha = host(acc, n), hd = host(view_dirs, 3 * n * V);
        auto single = restate<float>(wv, host_params[13], host_params[14], host_params[15], feature, hw, ha, hd, n, S, V, bf);
        auto exact = restate<double>(wv, host_params[13], host_params[14], host_params[15], feature, hw, ha, hd, n, S, V, bf);
        double tolerance = 0.0;
        for (size_t i = 0; i < exact.size(); ++i) tolerance = std::fmax(tolerance, std::fabs((double)single[i] - exact[i]));
        tolerance *= 4.0;
        auto hs = host(swept, 3 * n * V), ho = host(ordinary, 3 * n * V), hg = host(again, 3 * n * V);
        double against_ordinary = 0.0, against_exact = 0.0, spread = 0.0, lowest_acc = 1.0;
        for (size_t i = 0; i < hs.size(); ++i) {
            CHECK(std::isfinite(hs[i]));
            CHECK(hg[i] == hs[i]);          // a second call: the same bits
            against_ordinary = std::fmax(against_ordinary, std::fabs((double)hs[i] - ho[i]));
            against_exact = std::fmax(against_exact, std::fabs((double)hs[i] - exact[i]));
        }
        for (size_t i = 0; i < (size_t)3 * n; ++i) spread = std::fmax(spread, std::fabs((double)hs[i] - hs[3 * n + i]));
        for (float v : ha) lowest_acc = std::fmin(lowest_acc, v);
        std::printf("view_sweep16_abi_smoke [%s]: against the ordinary sequence %.3e, against the double restatement %.3e, tolerance %.3e, "
                    "spread between two views %.3e, lowest acc %.3f\n", name, against_ordinary, against_exact, tolerance, spread, lowest_acc);
        CHECK(tolerance > 0.0 && tolerance < 1e-5);
        CHECK(against_exact <= tolerance);
        CHECK(against_ordinary <= tolerance);
        CHECK(spread > 100 * tolerance);         // the view directions matter
    }
    // refusals are status codes
    CHECK(snerf_view_sweep_half(&desc, params.data(), np, saved, weights, nullptr, view_dirs, n, S, V, 1, SNERF_PRECISION_BF16, again, work,
                                nullptr) == SNERF_E_INVALID);
    CHECK(snerf_view_sweep_half(&desc, params.data(), np, saved, weights, acc, view_dirs, n, S, V, 1, SNERF_PRECISION_FP32, again, work,
                                nullptr) == SNERF_E_INVALID);
    snerf_mlp_desc visible = desc;
    visible.predict_visibility = 1;
    CHECK(snerf_view_sweep_half_workspace_floats(&visible, n, S, V) == 0 && snerf_view_sweep_half_acts_floats(&visible, n, S) == 0);
    CHECK(snerf_view_sweep_half(&desc, params.data(), np, saved, weights, acc, view_dirs, 0, S, V, 1, SNERF_PRECISION_F16, again, work,
                                nullptr) == SNERF_OK);
    std::printf("view_sweep16_abi_smoke: OK\n");
    return 0;
}
