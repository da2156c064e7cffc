// The host compiler's layout of every struct of the C ABI (include/simplenerf_hip.h, include/simplenerf_train.h): one line
// "struct <name> <sizeof>" per struct and one line "<name>.<field> <offsetof> <sizeof>" per field, in declaration order.
// tests/test_abi_layout_host.py holds the ctypes classes the binding derives from the headers to these numbers.  A field
// missing here fails that test (the derived class has it); a field that does not exist fails to compile.
#include <cstddef>
#include <cstdio>

#include "simplenerf_hip.h"
#include "simplenerf_train.h"

#define STRUCT(type) std::printf("struct " #type " %zu\n", sizeof(type))
#define FIELD(type, field) std::printf(#type "." #field " %zu %zu\n", offsetof(type, field), sizeof(((type*)nullptr)->field))

int main() {
    STRUCT(snerf_mlp_desc);
    FIELD(snerf_mlp_desc, points_net_depth);
    FIELD(snerf_mlp_desc, points_net_width);
    FIELD(snerf_mlp_desc, views_net_depth);
    FIELD(snerf_mlp_desc, views_net_width);
    FIELD(snerf_mlp_desc, points_pe_degree);
    FIELD(snerf_mlp_desc, views_pe_degree);
    FIELD(snerf_mlp_desc, sigma_pe_degree);
    FIELD(snerf_mlp_desc, use_view_dirs);
    FIELD(snerf_mlp_desc, view_dependent_rgb);
    FIELD(snerf_mlp_desc, predict_visibility);

    STRUCT(snerf_render_config);
    FIELD(snerf_render_config, ndc);
    FIELD(snerf_render_config, white_bkgd);
    FIELD(snerf_render_config, lindisp);
    FIELD(snerf_render_config, num_coarse);
    FIELD(snerf_render_config, num_fine);
    FIELD(snerf_render_config, precision);
    FIELD(snerf_render_config, keep_activations);
    FIELD(snerf_render_config, fused);

    STRUCT(snerf_render_mlp);
    FIELD(snerf_render_mlp, desc);
    FIELD(snerf_render_mlp, packed);

    STRUCT(snerf_render_rays);
    FIELD(snerf_render_rays, rays_o);
    FIELD(snerf_render_rays, rays_d);
    FIELD(snerf_render_rays, view_dirs);
    FIELD(snerf_render_rays, rays_o_ndc);
    FIELD(snerf_render_rays, rays_d_ndc);
    FIELD(snerf_render_rays, near);
    FIELD(snerf_render_rays, far);
    FIELD(snerf_render_rays, t_rand);
    FIELD(snerf_render_rays, u);
    FIELD(snerf_render_rays, sigma_noise);
    FIELD(snerf_render_rays, depths_fine);
    FIELD(snerf_render_rays, rays_o2);
    FIELD(snerf_render_rays, num_other);

    STRUCT(snerf_render_level_out);
    FIELD(snerf_render_level_out, rgb);
    FIELD(snerf_render_level_out, acc);
    FIELD(snerf_render_level_out, depth);
    FIELD(snerf_render_level_out, depth_var);
    FIELD(snerf_render_level_out, depth_ndc);
    FIELD(snerf_render_level_out, depth_var_ndc);
    FIELD(snerf_render_level_out, alpha);
    FIELD(snerf_render_level_out, visibility);
    FIELD(snerf_render_level_out, weights);
    FIELD(snerf_render_level_out, sigma);
    FIELD(snerf_render_level_out, raw_rgb);
    FIELD(snerf_render_level_out, saved_acts);
    FIELD(snerf_render_level_out, raw_visibility);
    FIELD(snerf_render_level_out, raw_visibility2);
    FIELD(snerf_render_level_out, visibility2);
    FIELD(snerf_render_level_out, view_dirs2);

    STRUCT(snerf_render_outputs);
    FIELD(snerf_render_outputs, depths_coarse);
    FIELD(snerf_render_outputs, depths_fine);
    FIELD(snerf_render_outputs, level);

    STRUCT(snerf_render_level_grads);
    FIELD(snerf_render_level_grads, rgb);
    FIELD(snerf_render_level_grads, acc);
    FIELD(snerf_render_level_grads, depth);
    FIELD(snerf_render_level_grads, depth_ndc);
    FIELD(snerf_render_level_grads, sigma);
    FIELD(snerf_render_level_grads, raw_rgb);
    FIELD(snerf_render_level_grads, param_grads);
    FIELD(snerf_render_level_grads, num_params);
    FIELD(snerf_render_level_grads, accumulate);

    STRUCT(snerf_render_slot);
    FIELD(snerf_render_slot, unit_offset);
    FIELD(snerf_render_slot, present);
    FIELD(snerf_render_slot, returned);
    FIELD(snerf_render_slot, pool);
    FIELD(snerf_render_slot, rank);
    FIELD(snerf_render_slot, dims);

    STRUCT(snerf_render_layout);
    FIELD(snerf_render_layout, num_fine);
    FIELD(snerf_render_layout, samples);
    FIELD(snerf_render_layout, needs_workspace);
    FIELD(snerf_render_layout, pool_unit_floats);
    FIELD(snerf_render_layout, depths_coarse);
    FIELD(snerf_render_layout, depths_fine);
    FIELD(snerf_render_layout, level);

    STRUCT(snerf_loss_term);
    FIELD(snerf_loss_term, pred);
    FIELD(snerf_loss_term, target);
    FIELD(snerf_loss_term, numerator_mask);
    FIELD(snerf_loss_term, denominator_mask);
    FIELD(snerf_loss_term, d_pred);
    FIELD(snerf_loss_term, channels);
    FIELD(snerf_loss_term, group);
    FIELD(snerf_loss_term, accumulate);
    FIELD(snerf_loss_term, weight);
    FIELD(snerf_loss_term, d_target);
    FIELD(snerf_loss_term, accumulate_target);

    STRUCT(snerf_batch);
    FIELD(snerf_batch, rays_o);
    FIELD(snerf_batch, rays_d);
    FIELD(snerf_batch, view_dirs);
    FIELD(snerf_batch, rays_o_ndc);
    FIELD(snerf_batch, rays_d_ndc);
    FIELD(snerf_batch, pixel_id);
    FIELD(snerf_batch, target_rgb);
    FIELD(snerf_batch, near);
    FIELD(snerf_batch, far);
    FIELD(snerf_batch, near_ndc);
    FIELD(snerf_batch, far_ndc);
    FIELD(snerf_batch, sparse_depth_values);
    FIELD(snerf_batch, sparse_depth_errors);
    FIELD(snerf_batch, sparse_depth_values_ndc);
    FIELD(snerf_batch, mask_pixel_rays);
    FIELD(snerf_batch, mask_sparse_rays);
    FIELD(snerf_batch, global_rows);

    STRUCT(snerf_iteration);
    FIELD(snerf_iteration, iter_num);
    FIELD(snerf_iteration, pixel_epoch);
    FIELD(snerf_iteration, pixel_first);
    FIELD(snerf_iteration, sparse_epoch);
    FIELD(snerf_iteration, sparse_first);
    FIELD(snerf_iteration, adam_neg_step_size);
    FIELD(snerf_iteration, adam_bias2_sqrt);
    FIELD(snerf_iteration, reserved);
    return 0;
}
