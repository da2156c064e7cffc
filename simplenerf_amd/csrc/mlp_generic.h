// The layered MLP path (mlp_generic.hip): plan + entry points used by the C-ABI functions when build_plan (mlp_plan.h)
// reports a shape the fused kernels are not built for.
#pragma once
#include <algorithm>
#include <vector>

#include "snerf_common.h"

namespace snerf {

struct GenericPlan {
    int depth = 0, width = 0, views_depth = 0, views_width = 0;
    bool view_dep = false;
    int points_degree = 0, views_degree = 0;
    int pe_full = 0, pts_in = 0, extra = 0, views_pe = 0, views_in = 0, pts_out_rows = 1;
    int num_params = 0;
    std::vector<long long> w_off, w_count;   // parameter i in the "packed" buffer (ABI order, plain copies)
    long long packed_floats = 0;
    long long row = 0;                       // floats per sample of the fp32 activation row: the matrix of either format fits in N x row
    bool skip_layer(int l) const { return l == 5 && depth > 5; }   // its input is [encoding | H_4] (:580, :662-663)
    int layer_in_dim(int l) const { return l == 0 ? pts_in : (skip_layer(l) ? pts_in + width : width); }
};

// The activation row of one operand format (elements of that format per sample).  Blocks in layer order, each starting at a multiple
// of `align` elements (16 bytes: the GEMMs stage 16 bytes at a time); the skip layer's input is ONE block [encoding | H_4].  The
// heads' fp32 outputs are columns c_out.. and c_vout.. of rows head_rs floats apart: of the row itself (heads_in_row: fp32), or of
// an fp32 [N][8] block after the matrix (bf16).
struct GenericRow {
    long long row = 0;
    int c_pe = 0, c_pev = 0, c_x5 = -1, c_v0 = 0;
    std::vector<int> c_h, c_hv;
    int c_out = 0, c_vout = 4;
    long long head_rs = 8;
    int layer_in_col(const GenericPlan& p, int l) const { return l == 0 ? c_pe : (p.skip_layer(l) ? c_x5 : c_h[l - 1]); }
};

int generic_plan(const snerf_mlp_desc* desc, GenericPlan* out);
GenericRow generic_row(const GenericPlan& p, int align, bool heads_in_row);
int generic_pack(const GenericPlan& p, const float* const* params, float* packed, hipStream_t stream);
size_t generic_saved_floats(const GenericPlan& p, long long total);
int generic_forward(const GenericPlan& p, const float* packed, const float* origins, const float* dirs, const float* view_dirs,
                    const float* depths, long long num_rays, int num_samples, const float* noise, float* sigma, float* rgb,
                    float* saved_acts, int precision, hipStream_t stream);
size_t generic_backward_workspace_floats(const GenericPlan& p, long long total);
int generic_backward(const GenericPlan& p, const float* packed, const float* acts, const float* sigma, const float* rgb,
                     const float* d_sigma, const float* d_rgb, long long total, float* workspace, float* const* grads, int precision,
                     int accumulate, hipStream_t stream);

// the same two calls on bf16 operands (mlp_generic_bf16.hip), routed there by generic_forward / generic_backward
int generic_forward_bf16(const GenericPlan& p, const float* packed, const float* origins, const float* dirs, const float* view_dirs,
                         const float* depths, long long num_rays, int num_samples, const float* noise, float* sigma, float* rgb,
                         float* saved_acts, hipStream_t stream);
int generic_backward_bf16(const GenericPlan& p, const float* packed, const float* acts, const float* sigma, const float* rgb,
                          const float* d_sigma, const float* d_rgb, long long total, float* workspace, float* const* grads,
                          int accumulate, hipStream_t stream);

// scratch of the inference forward (host_state.hip): a block of at least `floats` of the (device, stream) whose lock the caller holds
int generic_arena(const StreamLock& held, size_t floats, float** out);

// row chunks the weight-gradient products of the backward are split into (fixed-order reduction)
inline int generic_wgrad_splits(long long total) { return (int)std::min<long long>(64, std::max<long long>(1, total / 8192)); }

// build_plan said "unsupported": is it a shape the layered path takes?  (fills *plan when so)
inline bool generic_takes(const snerf_mlp_desc* desc, GenericPlan* plan) { return generic_plan(desc, plan) == SNERF_OK; }

}  // namespace snerf
