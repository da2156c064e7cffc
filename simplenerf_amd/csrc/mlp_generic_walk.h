// The layer walk of the layered MLP path, written once for its two operand formats: fp32 (mlp_generic.hip) and bf16
// (mlp_generic_bf16.hip), each of which instantiates it.  The walk owns the network's topology: the encoding, the trunk with its
// skip layer, the density head, feature -> views chain -> colour head, the heads; in the backward the reverse order, the ping-pong
// of the dZ buffers, which activation gates which input gradient, the skip layer's column offset, and every parameter index.
// A format `Ops` supplies only what differs:
//   Act                       element type of the activation matrix and of the dZ buffers (float, or bf16 bits)
//   kName                     what its launch errors are called
//   kAlign, kHeadsInRow       its activation row (generic_row)
//   ld(width)                 row stride of a dZ buffer of `width` columns
//   floats(elems)             floats that a buffer of `elems` Act takes
//   linear                    Y = act(X . W^T + b) of the forward
//   input_grad                dX (+)= dZ . W[:, cols], gated by the ReLU of the layer that produced X
//   wgrad_gemm                the split-K partial sums of dW = dZ^T . X
//   colsum                    the partial column sums of dZ (bias gradient), for a layer's dZ (Act) or a head's (fp32)
// Everything sits in an unnamed namespace, as in mlp_generic_kernels.h: each translation unit has its own copy.
#pragma once
#include <algorithm>

#include "mlp_generic.h"
#include "mlp_generic_kernels.h"

namespace {

using snerf::GenericPlan;
using snerf::GenericRow;

// The output tile of a GEMM of either format: 128 x 128 where the product is at least 128 x 128 and the large tiles still fill the
// chip twice over (a 256 x 256 weight gradient split 32 ways is 128 workgroups of 128 x 128: 22.6 -> 25.5 ms for the 8 x 256 /
// 2 x 128 backward before this condition), 64 x 64 elsewhere.  Each output element is one fp32 chain over k in order whatever the
// tile: the tile only decides which workgroup computes it.
inline dim3 gemm_grid(int M, int N, int splits, int* tile) {
    const long long large_tiles = (long long)((N + 127) / 128) * ((M + 127) / 128) * (splits > 0 ? splits : 1);
    *tile = M >= 128 && N >= 128 && large_tiles >= 512 ? 128 : 64;
    return dim3((N + *tile - 1) / *tile, (M + *tile - 1) / *tile, splits > 0 ? splits : 1);
}

inline bool aligned16(const void* ptr) { return reinterpret_cast<uintptr_t>(ptr) % 16 == 0; }

template <class Ops>
int launched(const char* step) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SNERF_OK : snerf::fail(SNERF_E_HIP, "%s(%s): %s", Ops::kName, step, hipGetErrorString(e));
}

// forward over `total` consecutive samples starting at sample `first` of the call (a ray boundary); acts: `total` rows of the
// activation matrix, within generic_saved_floats(total)
template <class Ops>
int forward_rows(const GenericPlan& p, const float* packed, const float* origins, const float* dirs, const float* view_dirs,
                 const float* depths, long long first, long long total, int samples, const float* noise, float* sigma, float* rgb,
                 float* acts_floats, hipStream_t s) {
    using Act = typename Ops::Act;
    const GenericRow r = snerf::generic_row(p, Ops::kAlign, Ops::kHeadsInRow);
    const long long matrix = Ops::floats(total * r.row);
    if (matrix + (Ops::kHeadsInRow ? 0 : 8 * total) > (long long)snerf::generic_saved_floats(p, total))
        return snerf::fail(SNERF_E_UNSUPPORTED, "%s: activation row of %lld elements and the heads exceed %lld floats", Ops::kName, r.row, p.row);
    Act* acts = reinterpret_cast<Act*>(acts_floats);
    float* heads = Ops::kHeadsInRow ? acts_floats : acts_floats + matrix;
    EncodeArgs e = {};
    e.origins = origins + (first / samples) * 3; e.dirs = dirs + (first / samples) * 3;
    e.view_dirs = view_dirs ? view_dirs + (first / samples) * 3 : nullptr;
    e.depths = depths + first; e.acts = acts; e.row = r.row; e.total = total; e.samples = samples;
    e.points_degree = p.points_degree; e.views_degree = p.views_degree; e.pe_full = p.pe_full; e.pts_in = p.pts_in;
    e.views_pe = p.view_dep ? p.views_pe : 0;
    e.c_pe = r.c_pe; e.c_pev = r.c_pev; e.c_x5 = r.c_x5; e.c_v0_extra = p.view_dep && p.extra > 0 ? r.c_v0 + p.width : -1;
    e.c_v0_views = p.view_dep ? r.c_v0 + p.width + p.extra : -1;
    hipLaunchKernelGGL(encode_kernel<Act>, dim3(snerf::stride_grid(total * (p.pe_full + (p.view_dep ? p.views_pe : 0)), 256)), dim3(256), 0,
                       s, e);
    int rc = launched<Ops>("encode");
    if (rc != SNERF_OK) return rc;
    for (int l = 0; l < p.depth; ++l) {
        rc = Ops::linear(acts + r.layer_in_col(p, l), r.row, acts + r.c_h[l], r.row, total, p.layer_in_dim(l), p.width, packed + p.w_off[2 * l],
                         packed + p.w_off[2 * l + 1], true, s);
        if (rc != SNERF_OK) return rc;
    }
    const int po = 2 * p.depth;
    const Act* h_last = acts + r.c_h[p.depth - 1];
    rc = Ops::linear(h_last, r.row, heads + r.c_out, r.head_rs, total, p.width, p.pts_out_rows, packed + p.w_off[po], packed + p.w_off[po + 1],
                     false, s);
    if (rc != SNERF_OK) return rc;
    if (p.view_dep) {
        rc = Ops::linear(h_last, r.row, acts + r.c_v0, r.row, total, p.width, p.width, packed + p.w_off[po + 2], packed + p.w_off[po + 3], false,
                         s);                                                                       // feature: no activation (:683)
        if (rc != SNERF_OK) return rc;
        for (int j = 0; j < p.views_depth; ++j) {
            rc = Ops::linear(acts + (j == 0 ? r.c_v0 : r.c_hv[j - 1]), r.row, acts + r.c_hv[j], r.row, total, j == 0 ? p.views_in : p.views_width,
                             p.views_width, packed + p.w_off[po + 4 + 2 * j], packed + p.w_off[po + 5 + 2 * j], true, s);
            if (rc != SNERF_OK) return rc;
        }
        const int pv = po + 4 + 2 * p.views_depth;
        rc = Ops::linear(acts + r.c_hv[p.views_depth - 1], r.row, heads + r.c_vout, r.head_rs, total, p.views_width, 3, packed + p.w_off[pv],
                         packed + p.w_off[pv + 1], false, s);
        if (rc != SNERF_OK) return rc;
    }
    hipLaunchKernelGGL(heads_kernel, dim3(snerf::stride_grid(total, 256)), dim3(256), 0, s, heads, r.head_rs, r.c_out, r.c_vout,
                       p.view_dep ? 1 : 0, noise ? noise + first : nullptr, total, sigma + first, rgb + first * 3);
    return launched<Ops>("heads");
}

constexpr long long kInferenceChunk = 65536;     // samples per pass of the inference forward (bounds its scratch)

// the whole forward: training (saved_acts) in one pass, inference in passes of whole rays through the stream's scratch block
template <class Ops>
int forward_call(const GenericPlan& p, const float* packed, const float* origins, const float* dirs, const float* view_dirs,
                 const float* depths, long long num_rays, int num_samples, const float* noise, float* sigma, float* rgb,
                 float* saved_acts, hipStream_t s) {
    if (saved_acts)
        return forward_rows<Ops>(p, packed, origins, dirs, view_dirs, depths, 0, num_rays * num_samples, num_samples, noise, sigma, rgb,
                                 saved_acts, s);
    const long long rays_per_chunk = std::max(1LL, kInferenceChunk / num_samples);
    // every pass of the call writes and reads the stream's one scratch block: no other thread's pass may come in between
    const snerf::StreamLock serialised(s);
    float* scratch = nullptr;
    const int rc = snerf::generic_arena(serialised, (size_t)std::min(num_rays, rays_per_chunk) * num_samples * p.row, &scratch);
    if (rc != SNERF_OK) return rc;
    for (long long ray = 0; ray < num_rays; ray += rays_per_chunk) {
        const long long rays = std::min(rays_per_chunk, num_rays - ray);
        const int st = forward_rows<Ops>(p, packed, origins, dirs, view_dirs, depths, ray * num_samples, rays * num_samples, num_samples,
                                         noise, sigma, rgb, scratch, s);
        if (st != SNERF_OK) return st;
    }
    return SNERF_OK;
}

// The backward's workspace, in floats: dZ ping-pong (two buffers of N rows of the widest layer) | d heads (dout, dvout: N x 4 fp32
// each) | split-K partial sums (fp32, splits x (biggest weight + widest)).  generic_backward_workspace_floats reports the fp32
// layout's end + 64; every format's must fit in that (checked per call).
struct Workspace {
    long long widest, biggest, dz, dout, dvout, partial, end;
    int splits;
};

template <class Ops>
Workspace workspace_of(const GenericPlan& p, long long total) {
    Workspace w;
    w.widest = std::max({p.width, p.views_width, p.views_in, p.pts_in + p.width});
    w.biggest = std::max({(long long)p.width * (p.pts_in + p.width), (long long)p.views_width * p.views_in,
                          (long long)p.views_width * p.views_width, (long long)p.width * p.width});
    w.splits = snerf::generic_wgrad_splits(total);
    w.dz = Ops::floats(total * Ops::ld(w.widest));
    w.dout = 2 * w.dz;
    w.dvout = w.dout + 4 * total;
    w.partial = w.dvout + 4 * total;
    w.end = w.partial + (long long)w.splits * (w.biggest + w.widest);
    return w;
}

template <class Ops>
int backward_walk(const GenericPlan& p, const float* packed, const float* acts_floats, const float* sigma, const float* rgb,
                  const float* d_sigma, const float* d_rgb, long long total, float* workspace, float* const* grads, int accumulate,
                  hipStream_t s) {
    using Act = typename Ops::Act;
    const GenericRow r = snerf::generic_row(p, Ops::kAlign, Ops::kHeadsInRow);
    const Workspace w = workspace_of<Ops>(p, total);
    if (w.end > (long long)snerf::generic_backward_workspace_floats(p, total))
        return snerf::fail(SNERF_E_UNSUPPORTED, "%s: backward workspace layout exceeds the reported size", Ops::kName);
    const Act* acts = reinterpret_cast<const Act*>(acts_floats);
    float* dout = workspace + w.dout;
    float* dvout = workspace + w.dvout;
    float* partial = workspace + w.partial;
    const long long k_chunk = (total + w.splits - 1) / w.splits;
    const long long ld_t = Ops::ld(p.width), ld_v = Ops::ld(p.views_width);      // row strides of the dZ buffers

    hipLaunchKernelGGL(heads_backward_kernel, dim3(snerf::stride_grid(total, 256)), dim3(256), 0, s, sigma, rgb, d_sigma, d_rgb, total,
                       p.view_dep ? 1 : 0, dout, dvout);
    int rc = launched<Ops>("heads backward");
    if (rc != SNERF_OK) return rc;

    // dW = dZ^T . X (split over the samples, fixed-order reduction), db = column sums of dZ; dZ Act (a layer) or fp32 (a head)
    auto weight_grad = [&](auto dz, long long dz_ld, int out, const Act* x, int in, float* gw, float* gb) -> int {
        int st = Ops::wgrad_gemm(dz, dz_ld, out, x, r.row, in, total, w.splits, k_chunk, partial, s);
        if (st != SNERF_OK) return st;
        hipLaunchKernelGGL(reduce_splits_kernel, dim3(snerf::stride_grid((long long)out * in, 256)), dim3(256), 0, s, partial,
                           (long long)out * in, w.splits, (long long)out * in, gw, accumulate);
        st = launched<Ops>("reduce");
        if (st != SNERF_OK) return st;
        // bias gradient = column sums of dZ.  The weight partial sums above have just been folded, so their area is free again: the
        // column sums take four times as many row chunks as the GEMM had splits (32 chunks x two column blocks was 64 workgroups on
        // 256 CUs: 151 us per call at 262 144 x 512, 3.6 TB/s) and put their partial rows at its start.
        const int bsplits = in >= 4 ? w.splits * 4 : w.splits;      // (the area holds splits x out x in floats: room for splits x in rows of `out`)
        const long long b_chunk = (total + bsplits - 1) / bsplits;
        st = Ops::colsum(dz, dz_ld, out, total, bsplits, b_chunk, partial, s);
        if (st == SNERF_OK) st = launched<Ops>("bias sums");
        if (st != SNERF_OK) return st;
        hipLaunchKernelGGL(reduce_splits_kernel, dim3(1), dim3(256), 0, s, partial, (long long)out, bsplits, (long long)out, gb, accumulate);
        return launched<Ops>("reduce bias");
    };
    // dX[:, cols] (+)= dZ . W[:, col0 : col0 + cols], then gated by the ReLU of the layer that produced X
    auto input_grad = [&](auto dz, long long dz_ld, int out, const float* wt, int w_ld, int col0, int cols, Act* dx, long long dx_ld,
                          bool add, const Act* gate) -> int {
        return Ops::input_grad(dz, dz_ld, out, wt + col0, w_ld, cols, dx, dx_ld, add, gate, r.row, total, s);
    };

    const int po = 2 * p.depth;
    Act* dh = reinterpret_cast<Act*>(workspace);      // gradient of the trunk's last activation H_D-1, then dZ of each trunk layer in turn
    Act* other = reinterpret_cast<Act*>(workspace + w.dz);
    const Act* h_last = acts + r.c_h[p.depth - 1];
    if (p.view_dep) {
        const int pv = po + 4 + 2 * p.views_depth;
        // views head and views layers, last first
        rc = weight_grad(dvout, 4, 3, acts + r.c_hv[p.views_depth - 1], p.views_width, grads[pv], grads[pv + 1]);
        if (rc != SNERF_OK) return rc;
        rc = input_grad(dvout, 4, 3, packed + p.w_off[pv], p.views_width, 0, p.views_width, other, ld_v, false, acts + r.c_hv[p.views_depth - 1]);
        if (rc != SNERF_OK) return rc;
        Act* dzv = other; Act* spare = dh;
        for (int j = p.views_depth - 1; j >= 0; --j) {
            const int in = j == 0 ? p.views_in : p.views_width;
            const Act* x = acts + (j == 0 ? r.c_v0 : r.c_hv[j - 1]);
            rc = weight_grad(dzv, ld_v, p.views_width, x, in, grads[po + 4 + 2 * j], grads[po + 5 + 2 * j]);
            if (rc != SNERF_OK) return rc;
            // j > 0: d HV_j-1, gated by its ReLU; j == 0: d feature = the first `width` columns of the views input (no activation)
            rc = input_grad(dzv, ld_v, p.views_width, packed + p.w_off[po + 4 + 2 * j], in, 0, j == 0 ? p.width : p.views_width, spare,
                            j == 0 ? ld_t : ld_v, false, j == 0 ? nullptr : acts + r.c_hv[j - 1]);
            if (rc != SNERF_OK) return rc;
            std::swap(dzv, spare);
        }
        Act* dfeature = dzv;          // (N, width)
        Act* dlast = spare;
        rc = weight_grad(dfeature, ld_t, p.width, h_last, p.width, grads[po + 2], grads[po + 3]);
        if (rc != SNERF_OK) return rc;
        rc = input_grad(dfeature, ld_t, p.width, packed + p.w_off[po + 2], p.width, 0, p.width, dlast, ld_t, false, nullptr);
        if (rc != SNERF_OK) return rc;
        dh = dlast; other = dfeature;
    }
    // density head (and the view-independent colour rows): dW_out, and its contribution to d H_D-1, then the ReLU gate
    rc = weight_grad(dout, 4, p.pts_out_rows, h_last, p.width, grads[po], grads[po + 1]);
    if (rc != SNERF_OK) return rc;
    rc = input_grad(dout, 4, p.pts_out_rows, packed + p.w_off[po], p.width, 0, p.width, dh, ld_t, p.view_dep, h_last);
    if (rc != SNERF_OK) return rc;
    // trunk, last layer first: dh holds dZ_l
    for (int l = p.depth - 1; l >= 0; --l) {
        const int in = p.layer_in_dim(l);
        rc = weight_grad(dh, ld_t, p.width, acts + r.layer_in_col(p, l), in, grads[2 * l], grads[2 * l + 1]);
        if (rc != SNERF_OK) return rc;
        if (l == 0) break;
        const int col0 = in - p.width;       // the skip layer's input is [encoding | H_l-1]: only the H columns carry on
        rc = input_grad(dh, ld_t, p.width, packed + p.w_off[2 * l], in, col0, p.width, other, ld_t, false, acts + r.c_h[l - 1]);
        if (rc != SNERF_OK) return rc;
        std::swap(dh, other);
    }
    return SNERF_OK;
}

}  // namespace
