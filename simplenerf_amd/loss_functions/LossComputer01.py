"""Training losses evaluated by the HIP library, behind the reference's ``LossComputer`` interface.

``LossComputer(configs).compute_losses(input_dict, output_dict, return_loss_maps=False)`` takes and returns what the
reference's class does (src/loss_functions/LossComputer01.py:12-53): a dictionary ``{loss name: {'loss_value': t},
'TotalLoss': t}`` whose ``TotalLoss.backward()`` drives the training step (src/Trainer01.py:93-96).  Thirteen of the
reference's fifteen loss classes are built: the nine every shipped experiment enables -- MSE01-03, SparseDepthMSE01-03,
PointsAugmentationDepthLoss02, ViewsAugmentationDepthLoss02, CoarseFineConsistencyLoss02 -- and the four its
experiment dictionaries carry commented out or behind the loader's ``dense_depth`` key:
PointsAugmentationDepthLoss01, ViewsAugmentationDepthLoss01, CoarseFineConsistencyLoss01 (plain MSE between two depth
estimates on every row of the batch, BOTH estimates receiving a gradient) and DenseDepthMSE01 (depth against a dense
prior on the pixel rays).  VisibilityLoss01 and VisibilityPriorLoss01 need a gradient through ``predict_visibility``,
which this build does not provide; they, and any other name, raise at construction, as an unknown module does in the
reference (:24-31).  So does a list whose terms cannot fit the table (``term_capacity``), naming the losses.

Instead of one Python object and a few dozen torch kernels per loss, every loss contributes rows to ONE table of
masked mean-squared-error terms; the table is evaluated by one launch (snerf_loss_forward) and differentiated by one
launch (snerf_loss_backward); the three patch-consistency losses add one launch each for their decision masks
(snerf_patch_consistency_masks).  See include/simplenerf_train.h.  There is no torch fallback.

Reference behaviour kept on purpose (pinned by tests/golden/losses_*.npz):
  * a mean over zero rays is 0, not NaN (MSE01.py:62);
  * SparseDepthMSE02/03 read ``depth_fine`` of the MAIN model when the augmentation has a fine MLP
    (SparseDepthMSE02.py:44);
  * of the two symmetric terms of a consistency loss only the one on the first estimate (main / coarse model) is
    non-zero: the reference computes the second from tensors its first call zeroed in place through ``detach()``
    aliases (PointsAugmentationDepthLoss02.py:172-173, :205-207), so it is identically zero in value and gradient.
    The augmented / fine depth therefore receives no gradient from these losses, here as there;
  * ``compute_losses`` replaces the tensors of ``input_dict['common_data']`` by their first (per-GPU) replica in
    place (LossComputer01.py:34-38).
  * DenseDepthMSE01 compares WORLD depth with ``dense_depth_values`` in NDC mode too and does not mask out the
    loader's -1 "no depth" entries (DenseDepthMSE01.py:29-30, :55-56).
One deliberate deviation: DenseDepthMSE01's fine branch reads ``self.num_rays``, which the reference's class never
sets (DenseDepthMSE01.py:40), so the reference raises AttributeError on any model with a fine MLP.  Here the slice is
the whole batch -- the only length for which its own expression ``pred[indices_mask]`` against
``gt_depth[indices_mask]`` is shape-consistent (tests/golden/losses01_dense_fine.npz was made by running the
reference's class with ``num_rays`` set to the batch length).
``CoarseFineConsistencyLoss01.compute_loss`` defaults ``return_loss_maps`` to True (CoarseFineConsistencyLoss01.py:24);
``compute_losses`` always passes the flag, so the default is never seen through this interface -- but without both
MLPs its result carries no ``loss_maps`` key even when maps are asked for (:29-33), here as there.
Loss maps (``return_loss_maps=True``, validation only) are assembled with torch ops from the kernel's masks -- off
the training path.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .. import ops

Tensor = torch.Tensor
_AUGMENTATION = {'01': '', '02': 'points_augmentation', '03': 'views_augmentation'}
_PATCH_LOSSES = {'PointsAugmentationDepthLoss02': 'points_augmentation', 'ViewsAugmentationDepthLoss02': 'views_augmentation',
                 'CoarseFineConsistencyLoss02': None}
# plain two-sided depth MSE: augmentation section of the model, or None for coarse against fine
_PLAIN_LOSSES = {'PointsAugmentationDepthLoss01': 'points_augmentation', 'ViewsAugmentationDepthLoss01': 'views_augmentation',
                 'CoarseFineConsistencyLoss01': None}
_DENSE_LOSS = 'DenseDepthMSE01'
SUPPORTED = tuple(f'{stem}{nn}' for stem in ('MSE', 'SparseDepthMSE') for nn in _AUGMENTATION) + tuple(_PATCH_LOSSES) \
    + tuple(_PLAIN_LOSSES) + (_DENSE_LOSS,)
MAX_TERMS = 16      # SNERF_LOSS_MAX_TERMS


def term_capacity(configs: dict) -> Dict[str, int]:
    """{loss name: the most table terms ``compute_losses`` can add for it} for ``configs['losses']`` on
    ``configs['model']`` -- a SparseDepthMSE term is counted although a batch without sparse-depth rays omits it."""
    model = configs['model']
    levels = lambda section: [level for level in ('coarse', 'fine') if f'{level}_mlp' in section]
    both = 'coarse_mlp' in model and 'fine_mlp' in model
    counts: Dict[str, int] = {}
    for loss_configs in configs['losses']:
        name = loss_configs['name']
        if name in _PATCH_LOSSES or name in _PLAIN_LOSSES:
            aug = _PATCH_LOSSES.get(name) or _PLAIN_LOSSES.get(name)
            if aug is None:
                count = int(both)
                if both and name in _PATCH_LOSSES and 'sparse_depth' in configs.get('data_loader', {}):
                    count += 1
            else:
                count = len([level for level in levels(model) if level in levels(model.get(aug, {}))])
        elif name == _DENSE_LOSS:
            count = len(levels(model))
        elif name.startswith('MSE'):
            aug = _AUGMENTATION[name[-2:]]
            count = len(levels(model.get(aug, {}) if aug else model))
        else:
            count = 1
        counts[name] = count
    return counts


class _FusedLossFunction(torch.autograd.Function):
    """values = snerf_loss_forward(table);  d pred = snerf_loss_backward(table, d values)."""

    @staticmethod
    def forward(ctx, terms, num_groups, owner, *unique_operands):
        """``owner[i]`` = (input index of term i's pred, input index of its target or None for a one-sided term)."""
        values, scales = ops.loss_forward(terms, num_groups)
        ctx.terms, ctx.num_groups, ctx.owner, ctx.scales = terms, num_groups, owner, scales
        return values

    @staticmethod
    def backward(ctx, grad_values):
        needs = ctx.needs_input_grad[3:]
        wanted = [needs[j] for j, _ in ctx.owner]
        wanted_target = [k is not None and needs[k] for _, k in ctx.owner]
        grads, target_grads = ops.loss_backward(ctx.terms, ctx.num_groups, ctx.scales, grad_values.contiguous(), wanted,
                                                wanted_target)
        per_input: List[Optional[Tensor]] = [None] * len(needs)
        # terms sharing an operand -- as pred of some, as differentiated target of others -- share one buffer that
        # already holds their sum
        for g, (j, _) in zip(grads, ctx.owner):
            if g is not None and per_input[j] is None:
                per_input[j] = g
        for g, (_, k) in zip(target_grads, ctx.owner):
            if g is not None and per_input[k] is None:
                per_input[k] = g
        return (None, None, None) + tuple(per_input)


class LossComputer:
    def __init__(self, configs: dict):
        self.configs = configs
        self.losses: Dict[str, dict] = {}
        for loss_configs in configs['losses']:
            name = loss_configs['name']
            if name not in SUPPORTED:
                raise RuntimeError(f'Unknown Loss Function: {name} (the HIP loss evaluation builds {", ".join(SUPPORTED)})')
            self.losses[name] = loss_configs
        if len(self.losses) > 16:
            raise RuntimeError('at most 16 losses fit the fused loss table')
        capacity = term_capacity({**configs, 'losses': list(self.losses.values())})
        if sum(capacity.values()) > MAX_TERMS:
            raise RuntimeError(f'the fused loss table holds {MAX_TERMS} terms; on this model the configured losses can take '
                               f'{sum(capacity.values())}: ' + ', '.join(f'{name} {count}' for name, count in capacity.items()))

    @staticmethod
    def get_loss_weight(loss_configs: dict, iter_num: int):
        """Constant ``weight`` or the ``iter_weights`` entry with the largest start <= iter_num (reference :55-69)."""
        weight = None
        if 'weight' in loss_configs:
            weight = loss_configs['weight']
        elif 'iter_weights' in loss_configs:
            for start in sorted((int(k) for k in loss_configs['iter_weights']), reverse=True):
                if iter_num >= start:
                    weight = loss_configs['iter_weights'][str(start)]
                    break
        if weight is None:
            raise RuntimeError(f"loss_weight is None for {loss_configs['name']} at iter {iter_num}")
        return weight

    # --------------------------------------------------------------------------------------------------
    def compute_losses(self, input_dict: dict, output_dict: dict, return_loss_maps: bool = False) -> dict:
        if 'common_data' in input_dict:
            common = input_dict['common_data']
            for key in common:
                if isinstance(common[key], torch.Tensor):
                    common[key] = common[key][0]
        model = self.configs['model']
        iter_num = input_dict['iter_num']
        mask_nerf = input_dict['indices_mask_nerf']
        mask_sd = input_dict.get('indices_mask_sparse_depth')
        terms: List[ops.LossTermSpec] = []
        operands: List[tuple] = []        # the caller's tensors (with their autograd history): (pred, target or None) per term
        maps: Dict[str, Optional[dict]] = {name: {} for name in self.losses}

        def add(group, weight, pred, target, numerator, denominator, two_sided=False):
            terms.append(ops.LossTermSpec(pred, target, numerator, denominator, group, weight, two_sided))
            operands.append((pred, target if two_sided else None))

        for group, (name, loss_configs) in enumerate(self.losses.items()):
            weight = self.get_loss_weight(loss_configs, iter_num)
            if name in _PATCH_LOSSES:
                self._patch_terms(name, loss_configs, group, weight, input_dict, output_dict, mask_nerf, mask_sd, add,
                                  maps[name] if return_loss_maps else None)
                continue
            if name in _PLAIN_LOSSES:
                maps[name] = self._plain_terms(name, group, weight, output_dict, add, return_loss_maps)
                continue
            if name == _DENSE_LOSS:
                gt_depth = input_dict['dense_depth_values'][:, 0]
                for level in ('coarse', 'fine'):
                    if f'{level}_mlp' in model:
                        add(group, weight, output_dict[f'depth_{level}'], gt_depth, mask_nerf, mask_nerf)
                        if return_loss_maps:
                            maps[name][f'{name}_{level}'] = torch.square(output_dict[f'depth_{level}'][mask_nerf] - gt_depth[mask_nerf])
                continue
            aug = _AUGMENTATION[name[-2:]]
            section = model[aug] if aug else model
            prefix = f'{aug}_' if aug else ''
            if name.startswith('MSE'):
                for level in ('coarse', 'fine'):
                    key = f'{prefix}rgb_{level}'
                    if f'{level}_mlp' in section and (not aug or key in output_dict):
                        add(group, weight, output_dict[key], input_dict['target_rgb'], mask_nerf, mask_nerf)
                        if return_loss_maps:
                            err = output_dict[key][mask_nerf] - input_dict['target_rgb'][mask_nerf]
                            maps[name][f'{name}_{level}'] = torch.mean(torch.square(err), dim=1)
            elif mask_sd is not None:     # SparseDepthMSE: only for batches that carry sparse-depth rays
                key = 'depth_fine' if 'fine_mlp' in section else f'{prefix}depth_coarse'
                add(group, weight, output_dict[key], input_dict['sparse_depth_values'][:, 0], mask_sd, mask_sd)

        num_groups = len(self.losses)
        device = input_dict['rays_o'].device
        if terms:
            unique: List[Tensor] = []

            def index_of(p: Optional[Tensor]) -> Optional[int]:
                if p is None:
                    return None
                for j, q in enumerate(unique):
                    if q is p:
                        return j
                unique.append(p)
                return len(unique) - 1

            owner = [(index_of(pred), index_of(target)) for pred, target in operands]
            values = _FusedLossFunction.apply(terms, num_groups, owner, *unique)
            count = len(terms)
        else:
            values = torch.zeros((num_groups + 1,), dtype=torch.float32, device=device)
            count = 0
        loss_values: Dict[str, object] = {}
        for group, name in enumerate(self.losses):
            loss_values[name] = {'loss_value': values[count + group]}
            if return_loss_maps and maps[name] is not None:
                loss_values[name]['loss_maps'] = maps[name]
        loss_values['TotalLoss'] = values[count + num_groups]
        return loss_values

    # --------------------------------------------------------------------------------------------------
    def _plain_terms(self, name, group, weight, output_dict, add, return_loss_maps) -> Optional[dict]:
        """The 01 consistency losses: mean squared difference of two depth estimates over EVERY row of the batch (no mask,
        sparse-depth rows included), both estimates differentiated -- one two-sided term per pair.  -> the loss maps
        (the per-ray squared error under the reference's keys), None where the reference's result has no such entry."""
        model = self.configs['model']
        aug = _PLAIN_LOSSES[name]
        if aug is None:
            if 'coarse_mlp' not in model or 'fine_mlp' not in model:
                return None
            depth1, depth2 = output_dict['depth_coarse'], output_dict['depth_fine']
            add(group, weight, depth1, depth2, None, None, two_sided=True)
            return {name: torch.square(depth1 - depth2)} if return_loss_maps else {}
        nested: Dict[str, Tensor] = {}
        for level in ('coarse', 'fine'):
            if f'{level}_mlp' in model and f'{level}_mlp' in model[aug]:
                depth1, depth2 = output_dict[f'depth_{level}'], output_dict[f'{aug}_depth_{level}']
                add(group, weight, depth1, depth2, None, None, two_sided=True)
                if return_loss_maps:
                    nested[f'{name}_{level}'] = torch.square(depth1 - depth2)
        return {name: nested}

    def _patch_terms(self, name, loss_configs, group, weight, input_dict, output_dict, mask_nerf, mask_sd, add, maps):
        model = self.configs['model']
        aug = _PATCH_LOSSES[name]
        if aug is None:
            if 'coarse_mlp' not in model or 'fine_mlp' not in model:
                return
            pairs = [('depth_coarse', 'depth_fine', f'{name}_coarse', f'{name}_fine')]
        else:
            pairs = [(f'depth_{level}', f'{aug}_depth_{level}', f'{name}_{level}_main', f'{name}_{level}_augmented')
                     for level in ('coarse', 'fine') if f'{level}_mlp' in model and f'{level}_mlp' in model[aug]]
        common = input_dict['common_data']
        h, w = common['resolution']
        if tuple(common['images'].shape[1:3]) != (int(h), int(w)):
            raise RuntimeError(f"common_data images {tuple(common['images'].shape)} do not match resolution {(h, w)}")
        for key1, key2, map1_name, map2_name in pairs:
            depth1, depth2 = output_dict[key1], output_dict[key2]
            _, better2 = ops.patch_consistency_masks(
                input_dict['rays_o'], input_dict['rays_d'], depth1, depth2, mask_nerf, input_dict['pixel_id'],
                common['poses'], common['intrinsics'][0], common['images'], loss_configs['patch_size'],
                loss_configs['rmse_threshold'])
            # estimate 1 is pulled towards estimate 2 where 2 reprojects better; mean over ALL pixel rays
            add(group, weight, depth1, depth2, better2, mask_nerf)
            if maps is not None:
                keep = better2[mask_nerf].to(depth1.dtype)
                maps[map1_name] = torch.square((depth1[mask_nerf] - depth2[mask_nerf].detach()) * keep)
                maps[map2_name] = torch.zeros_like(maps[map1_name])
        if aug is None and 'sparse_depth' in self.configs['data_loader'] and mask_sd is not None:
            add(group, weight, output_dict['depth_coarse'], output_dict['depth_fine'], mask_sd, mask_sd)
