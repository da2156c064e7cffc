// The output layout of a render call (snerf_render_layout, include/simplenerf_hip.h): which outputs a call has, their shapes,
// and where each lies in the per-ray and the per-sample pool.  This header is the ONE place that knows it: render.hip exports
// it, both host bindings allocate and carve from it.  Plain C++ with no HIP types, so that a host program can walk it
// (tests/native/render_layout_test.cpp, under AddressSanitizer).
//
// Order inside the per-sample pool: depths_coarse, [depths_fine], then per present level [alpha][visibility][weights], sigma,
// raw_rgb, [raw_visibility], [raw_visibility2, view_dirs2, hidden weights].  Inside the per-ray pool, per present level: rgb, acc,
// depth, depth_var, [depth_ndc, depth_var_ndc], [visibility2].
#pragma once

#include <cstddef>
#include <initializer_list>

#include "simplenerf_hip.h"

namespace snerf {
namespace renderlayout {

// the fields of snerf_render_level_out in the order of enum snerf_render_field
constexpr float* snerf_render_level_out::* kField[] = {
    &snerf_render_level_out::rgb, &snerf_render_level_out::acc, &snerf_render_level_out::depth, &snerf_render_level_out::depth_var,
    &snerf_render_level_out::depth_ndc, &snerf_render_level_out::depth_var_ndc, &snerf_render_level_out::alpha,
    &snerf_render_level_out::visibility, &snerf_render_level_out::weights, &snerf_render_level_out::sigma,
    &snerf_render_level_out::raw_rgb, &snerf_render_level_out::saved_acts, &snerf_render_level_out::raw_visibility,
    &snerf_render_level_out::raw_visibility2, &snerf_render_level_out::visibility2, &snerf_render_level_out::view_dirs2};
static_assert(sizeof(kField) / sizeof(kField[0]) == SNERF_RENDER_FIELDS && SNERF_FIELD_VIEW_DIRS2 + 1 == SNERF_RENDER_FIELDS &&
                  sizeof(snerf_render_level_out) == SNERF_RENDER_FIELDS * sizeof(float*),
              "snerf_render_level_out, enum snerf_render_field and kField list the same fields");

// Samples per ray of a level: the coarse levels 0-2 march num_coarse depths, the fine levels 3-5 the merged num_coarse + num_fine.
inline int samples(int num_coarse, int num_fine, int level) { return level < SNERF_LEVEL_MAIN_FINE ? num_coarse : num_coarse + num_fine; }
inline int samples(const snerf_render_config* cfg, int level) { return samples(cfg->num_coarse, cfg->num_fine, level); }

// Fills `lay`; returns NULL, or what is wrong with the arguments.
inline const char* query(const snerf_render_config* cfg, const snerf_render_mlp* mlps, int num_other, int per_sample_mask,
                         bool fine_depths_given, snerf_render_layout* lay) {
    if (!cfg || !mlps || !lay) return "NULL argument";
    if (cfg->num_coarse < 1 || cfg->num_fine < 0) return "bad sample counts";
    if (num_other < 0) return "negative num_other";
    if (per_sample_mask < 0 || per_sample_mask > 7) return "per_sample_mask is 1 alpha | 2 visibility | 4 weights";
    if (!mlps[SNERF_LEVEL_MAIN_COARSE].desc) return "the main coarse MLP is required";
    *lay = snerf_render_layout{};
    const bool fine = mlps[SNERF_LEVEL_MAIN_FINE].desc != nullptr;
    lay->num_fine = fine ? cfg->num_fine : 0;
    lay->needs_workspace = fine && !fine_depths_given && !(per_sample_mask & 4);      // the main coarse weights feed the resampling
    // the next free place of its pool
    auto put = [lay](snerf_render_slot& slot, int pool, bool returned, std::initializer_list<int> dims) {
        slot.present = 1;
        slot.returned = returned;
        slot.pool = pool;
        long long unit = 1;
        for (int d : dims) { slot.dims[slot.rank++] = d; unit *= d; }
        if (pool == SNERF_POOL_OWN) return;
        slot.unit_offset = lay->pool_unit_floats[pool];
        lay->pool_unit_floats[pool] += unit;
    };
    const int ray = SNERF_POOL_PER_RAY, sample = SNERF_POOL_PER_SAMPLE, k = num_other;
    for (int l = 0; l < SNERF_RENDER_LEVELS; ++l) lay->samples[l] = samples(cfg->num_coarse, lay->num_fine, l);
    put(lay->depths_coarse, sample, true, {lay->samples[SNERF_LEVEL_MAIN_COARSE]});
    if (fine && !fine_depths_given) put(lay->depths_fine, sample, true, {lay->samples[SNERF_LEVEL_MAIN_FINE]});
    for (int l = 0; l < SNERF_RENDER_LEVELS; ++l) {
        const int s = lay->samples[l];
        if (!mlps[l].desc) continue;
        snerf_render_slot* f = lay->level[l];
        put(f[SNERF_FIELD_RGB], ray, true, {3});
        put(f[SNERF_FIELD_ACC], ray, true, {});
        put(f[SNERF_FIELD_DEPTH], ray, true, {});
        put(f[SNERF_FIELD_DEPTH_VAR], ray, true, {});
        if (cfg->ndc) {
            put(f[SNERF_FIELD_DEPTH_NDC], ray, true, {});
            put(f[SNERF_FIELD_DEPTH_VAR_NDC], ray, true, {});
        }
        if (per_sample_mask & 1) put(f[SNERF_FIELD_ALPHA], sample, true, {s});
        if (per_sample_mask & 2) put(f[SNERF_FIELD_VISIBILITY], sample, true, {s});
        if (per_sample_mask & 4) put(f[SNERF_FIELD_WEIGHTS], sample, true, {s});
        put(f[SNERF_FIELD_SIGMA], sample, true, {s, 1});
        put(f[SNERF_FIELD_RAW_RGB], sample, true, {s, 3});
        if (mlps[l].desc->predict_visibility) {
            put(f[SNERF_FIELD_RAW_VISIBILITY], sample, true, {s, 1});
            if (k > 0) {
                put(f[SNERF_FIELD_RAW_VISIBILITY2], sample, true, {s, k, 1});
                put(f[SNERF_FIELD_VISIBILITY2], ray, true, {k});
                put(f[SNERF_FIELD_VIEW_DIRS2], sample, false, {s, k, 3});
                // visibility2 is composited with the level's weights: room for them when the caller did not ask for them
                if (!f[SNERF_FIELD_WEIGHTS].present) put(f[SNERF_FIELD_WEIGHTS], sample, false, {s});
            }
        }
        if (cfg->keep_activations) put(f[SNERF_FIELD_SAVED_ACTS], SNERF_POOL_OWN, false, {});
    }
    return nullptr;
}

inline void bind(const snerf_render_layout* lay, long long n, float* per_ray_pool, float* per_sample_pool, snerf_render_outputs* out) {
    float* const pools[2] = {per_ray_pool, per_sample_pool};
    auto at = [&](const snerf_render_slot& slot) -> float* {
        return slot.present && slot.pool != SNERF_POOL_OWN ? pools[slot.pool] + n * slot.unit_offset : nullptr;
    };
    out->depths_coarse = at(lay->depths_coarse);
    out->depths_fine = at(lay->depths_fine);
    for (int l = 0; l < SNERF_RENDER_LEVELS; ++l)
        for (int f = 0; f < SNERF_RENDER_FIELDS; ++f) out->level[l].*kField[f] = at(lay->level[l][f]);
}

// The workspace of snerf_render_backward, in floats: per level the gradient columns d_sigma (n s_l) and d_rgb (3 n s_l) and the
// inner workspace of the level's MLP backward.  The ONE place that knows the partition: snerf_render_backward_workspace_floats
// sizes the allocation with it, snerf_render_backward carves it.
//   in order (the levels run one after the other and share one region): [ d_sigma | d_rgb | inner ] sized for the largest level,
//       4 max_l(n s_l) + max_l(inner_l);
//   side by side (each present level its own region, in level order): 4 n s_l + round_up(inner_l, 64) per level.
// A call sized side by side but run in order (one level wanted, no side streams to be had) carves the in-order offsets, which
// depend on the sample counts only, out of the larger allocation.
struct BackwardRegions {
    size_t d_sigma[SNERF_RENDER_LEVELS], d_rgb[SNERF_RENDER_LEVELS], inner[SNERF_RENDER_LEVELS];   // offsets; 0 for absent levels
    size_t total;
};

inline BackwardRegions backward_regions(const int (&samples)[SNERF_RENDER_LEVELS], const bool (&present)[SNERF_RENDER_LEVELS],
                                        const size_t (&inner_floats)[SNERF_RENDER_LEVELS], long long n, bool side_by_side) {
    BackwardRegions r = {};
    size_t columns_max = 0, inner_max = 0;
    for (int l = 0; l < SNERF_RENDER_LEVELS; ++l) {
        if (!present[l]) continue;
        const size_t columns = (size_t)n * (size_t)samples[l];
        if (columns > columns_max) columns_max = columns;
        if (inner_floats[l] > inner_max) inner_max = inner_floats[l];
        if (!side_by_side) continue;
        r.d_sigma[l] = r.total;
        r.d_rgb[l] = r.total + columns;
        r.inner[l] = r.total + 4 * columns;
        r.total += 4 * columns + (inner_floats[l] + 63) / 64 * 64;
    }
    if (side_by_side) return r;
    for (int l = 0; l < SNERF_RENDER_LEVELS; ++l) {
        if (!present[l]) continue;
        r.d_rgb[l] = columns_max;
        r.inner[l] = 4 * columns_max;
    }
    r.total = 4 * columns_max + inner_max;
    return r;
}

}  // namespace renderlayout
}  // namespace snerf
