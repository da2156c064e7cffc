#!/usr/bin/env python3
"""G10: golden vectors for the plain (01) depth losses and dense-depth supervision, made by RUNNING THE REFERENCE's
classes here: PointsAugmentationDepthLoss01, ViewsAugmentationDepthLoss01, CoarseFineConsistencyLoss01 and
DenseDepthMSE01 behind its LossComputer, and -- for the batch keys -- DataPreprocessor.load_dense_depth_cached_batch.

    PYTHONDONTWRITEBYTECODE=1 python3 tools/make_golden_losses01.py

Inputs come from the build-owned generators (``synth.loss01_case``: seeds and sizes are ``synth.LOSS01_CASES``); each
``tests/golden/losses01_<case>.npz`` stores the reference's loss values, ``TotalLoss``, the gradient of ``TotalLoss`` with
respect to every model output and (where the reference's own loss-map path runs) the per-ray loss maps, nested keys joined
by '/'.

Cases:  world       MSE01-03, SparseDepthMSE01-03 and the three 01 consistency losses at weight 0.1, world-space rays
        ndc         the same, NDC configuration, other seeds
        early       `world` at iteration 0 (consistency weights 0)
        dense       + DenseDepthMSE01 on a model WITHOUT a fine MLP (CoarseFineConsistencyLoss01 contributes 0)
        dense_fine  all thirteen losses (the nine shipped ones + the four) on the shipped model, NDC: 16 table terms
        empty       pixel-ray mask all false (8 sparse rays only): DenseDepthMSE01 is 0, the consistency losses are not

DenseDepthMSE01's fine branch reads ``self.num_rays``, which the reference's class never sets (DenseDepthMSE01.py:40): as
shipped it raises AttributeError on any model with a fine MLP.  For `dense_fine` and `empty` THIS GENERATOR SETS
``num_rays`` ON THE REFERENCE'S OBJECT TO THE BATCH LENGTH before calling it -- the only length for which the class's own
``pred[:num_rays][indices_mask]`` is shape-consistent with ``gt_depth[indices_mask]``; nothing else of the class is touched.

``tests/golden/batch_dense_depth.npz``: a train-mode DataPreprocessor with ``data_loader.dense_depth`` over the synthetic
scene of tools/make_golden_batch.py, NDC and world; per mode the dense tables it prepared (the weight table once: it is the
same in both), the indices it drew and the three dense-depth batch tensors of consecutive batches (sparse-depth rows included: they hold -1).
"""
import os
import sys
import types

import numpy
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tools'))
sys.path.insert(0, os.path.join(REF, 'src'))
for name in ('skimage', 'skimage.io', 'skimage.transform'):
    sys.modules.setdefault(name, types.ModuleType(name))

from data_preprocessors.DataPreprocessor01 import DataPreprocessor  # noqa: E402  (the reference)
from loss_functions.LossComputer01 import LossComputer  # noqa: E402  (the reference)

import make_golden_batch  # noqa: E402  (its synthetic raw scene and loader configs)
from simplenerf_amd import synth  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')


def flatten(prefix, maps, arrays):
    for key, value in maps.items():
        if isinstance(value, dict):
            flatten(f'{prefix}/{key}', value, arrays)
        else:
            arrays[f'{prefix}/{key}'] = value.detach().numpy()


def run_case(name):
    case = synth.LOSS01_CASES[name]
    configs, scene, batch, keys = synth.loss01_case(name)
    t = lambda a: torch.from_numpy(numpy.ascontiguousarray(a))
    input_dict = {
        'iter_num': case['iter_num'],
        'rays_o': t(batch['rays_o']), 'rays_d': t(batch['rays_d']), 'pixel_id': t(batch['pixel_id']),
        'target_rgb': t(batch['target_rgb']), 'indices_mask_nerf': t(batch['indices_mask_nerf']),
        'indices_mask_sparse_depth': t(batch['indices_mask_sparse_depth']), 'sparse_depth_values': t(batch['sparse_depth_values']),
        'common_data': {'poses': t(scene['poses'])[None], 'images': t(scene['images'])[None],
                        'intrinsics': t(scene['intrinsics'])[None], 'resolution': scene['resolution']},
    }
    if 'dense_depth_values' in batch:
        input_dict['dense_depth_values'] = t(batch['dense_depth_values'])
    output_dict = {k: t(batch[k]).clone().requires_grad_(True) for k in keys}
    computer = LossComputer(configs)
    if 'DenseDepthMSE01' in computer.losses and 'fine_mlp' in configs['model']:
        computer.losses['DenseDepthMSE01'].num_rays = batch['rays_o'].shape[0]      # see the module docstring
    # the 02 consistency losses' own loss-map path raises with sparse rows in the batch (tools/make_golden_losses.py)
    with_maps = not any(c['name'].endswith('Loss02') for c in configs['losses'])
    losses = computer.compute_losses(input_dict, output_dict, return_loss_maps=with_maps)
    total = losses['TotalLoss']
    arrays = {'TotalLoss': float(total), 'with_maps': with_maps}
    if isinstance(total, torch.Tensor) and total.requires_grad:
        total.backward()
    for k in keys:
        g = output_dict[k].grad
        arrays[f'grad_{k}'] = (g if g is not None else torch.zeros_like(output_dict[k])).numpy()
    for loss_name, entry in losses.items():
        if loss_name == 'TotalLoss':
            continue
        arrays[f'value_{loss_name}'] = float(entry['loss_value'])
        # the per-ray maps of the consistency losses are kept for two cases only (fixture size), DenseDepthMSE01's always
        if with_maps and ((name in ('world', 'dense') and loss_name.endswith('Loss01')) or loss_name == 'DenseDepthMSE01'):
            arrays[f'has_maps_{loss_name}'] = 'loss_maps' in entry
            flatten(f'map/{loss_name}', entry.get('loss_maps', {}), arrays)
    path = os.path.join(OUT, f'losses01_{name}.npz')
    numpy.savez_compressed(path, **arrays)
    print(f'losses01_{name}.npz: {os.path.getsize(path)} B; TotalLoss {float(total):.6f}; '
          + ', '.join(f"{k[6:]}={float(v):.5f}" for k, v in arrays.items() if k.startswith('value_')))
    print('   maps:', sorted(k for k in arrays if k.startswith('map/')))


def run_batches():
    arrays = {}
    for mode, ndc in (('ndc', True), ('world', False)):
        raw = make_golden_batch.raw_data()
        scene = synth.synth_scene(0)
        tables = synth.dense_depth_tables(scene, 0)
        v, (h, w) = 3, scene['resolution']
        raw['dense_depth_data'] = {'depth_values': tables['dense_depths'].reshape(v, h, w).astype(numpy.float64),
                                   'depth_weights': tables['dense_depth_weights'].reshape(v, h, w).astype(numpy.float64)}
        if not ndc:
            # world mode: near = bounds[0] * .9 stays a numpy scalar (DataPreprocessor01.py:146); as float64 it makes the
            # near/far columns float64 and the reference's own batch loader refuses them (:607)
            raw['nerf_data']['bounds'] = raw['nerf_data']['bounds'].astype(numpy.float32)
        numpy.random.seed(9)
        pp = DataPreprocessor(make_golden_batch.configs(ndc=ndc, sparse_depth={'num_rays': 32}, dense_depth={}), mode='train',
                              raw_data_dict=raw)
        dense = pp.preprocessed_data_dict['dense_depth_data']
        arrays[f'{mode}_dense_depths'] = dense['depth_values'].numpy().reshape(-1)
        if ndc:
            arrays['dense_depth_weights'] = dense['depth_weights'].numpy().reshape(-1)
        else:       # the weights are not rescaled: one copy serves both modes
            assert numpy.array_equal(arrays['dense_depth_weights'], dense['depth_weights'].numpy().reshape(-1))
        if ndc:
            arrays[f'{mode}_dense_depths_ndc'] = dense['depth_values_ndc'].numpy().reshape(-1)
        for b in range(2):
            batch = pp.get_next_batch(iter_num=b)
            arrays[f'{mode}_batch{b}_indices'] = batch['indices'].numpy()
            for key in ('dense_depth_values', 'dense_depth_weights', 'dense_depth_values_ndc'):
                assert (key in batch) == (ndc or not key.endswith('_ndc')), (mode, key)
                if key in batch:
                    arrays[f'{mode}_batch{b}_{key}'] = batch[key].numpy()
            assert int(batch['indices_mask_nerf'].sum()) == 96 and batch['indices'].shape[0] == 128
    path = os.path.join(OUT, 'batch_dense_depth.npz')
    numpy.savez_compressed(path, **arrays)
    print(f'batch_dense_depth.npz: {os.path.getsize(path)} B;', sorted(arrays))


if __name__ == '__main__':
    torch.set_num_threads(8)
    for case_name in synth.LOSS01_CASES:
        run_case(case_name)
    run_batches()
