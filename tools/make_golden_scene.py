#!/usr/bin/env python3
"""Golden vectors for the scene stage, made by RUNNING THE REFERENCE's DataPreprocessor on raw loader data.

    SIMPLENERF_REFERENCE_SRC=<reference checkout>/src PYTHONDONTWRITEBYTECODE=1 python3 tools/make_golden_scene.py

Three seeded 3-view scenes (``synth.raw_scene``; skimage is stubbed as in tools/make_golden_batch.py -- downsampling_factor is 1):
  scene_prep_ndc_sparse.npz   48x64, NDC, sparse depth: duplicate points (an exact repeat with another depth, three points on one
                              pixel), half-way coordinates (x = 2.5 and 3.5), points outside the frame on all four sides, and one
                              frame number missing from the dictionary
  scene_prep_world_dense.npz  37x53, world space, RGBA images on a white background, float32 dense depth with -1 entries,
                              recenter_camera_poses False
  scene_prep_ndc_both.npz     24x32, NDC, sparse and dense (float64) depth, bd_factor None
Each fixture holds the raw inputs, the reference's processed poses (train mode, and test mode from the saved model configs), sc,
average pose, near / far, float images, the sparse and dense tables, get_model_configs() as JSON, three batches with the index
lists the reference drew, and create_test_data of a held-out pose from a test-mode preprocessor built on those model configs.
"""
import copy
import json
import os
import sys
import types

import numpy
import pandas
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ['SIMPLENERF_REFERENCE_SRC'])       # the src/ directory of a checkout of the reference
for name in ('skimage', 'skimage.io', 'skimage.transform'):
    sys.modules.setdefault(name, types.ModuleType(name))

from data_preprocessors.DataPreprocessor01 import DataPreprocessor  # noqa: E402  (the reference)

from simplenerf_amd import synth  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
COLUMNS = ('x', 'y', 'depth', 'reprojection_error')


def configs(ndc, white_bkgd=False, **loader):
    return {'data_loader': {'bd_factor': 0.75, 'batching': True, 'ndc': ndc, 'downsampling_factor': 1, 'num_rays': 96,
                            'recenter_camera_poses': True, 'spherify': False, 'precrop_iterations': 0, **loader},
            'model': {'white_bkgd': white_bkgd}, 'device': 'cpu'}


def planted_points(height, width):
    """Rows (x, y, depth, error, what) appended to the first view's points, in this order."""
    return [
        (10.2, 5.4, 3.0, 0.5, 'repeat_first'), (10.2, 5.4, 4.5, 0.7, 'repeat_last'),          # an exact repeat: the later depth stays
        (20.1, 7.2, 3.1, 0.3, 'triple_a'), (19.9, 6.8, 3.2, 0.4, 'triple_b'), (20.4, 7.4, 3.3, 0.6, 'triple_c'),   # pixel (7, 20)
        (2.5, 12.0, 3.4, 0.2, 'half_down'), (3.5, 13.0, 3.5, 0.2, 'half_up'),                 # round half to even: columns 2 and 4
        (30.0, 0.5, 3.6, 0.2, 'half_row'), (31.0, -0.5, 3.7, 0.2, 'minus_half_row'),          # rows 0 and -0 -> 0
        (-3.2, 20.0, 3.8, 0.9, 'left'), (width + 5.3, 21.0, 3.9, 0.9, 'right'), (40.0, -1.7, 4.0, 0.9, 'above'),
        (41.0, height + 2.6, 4.1, 0.9, 'below'),                                              # clipped onto the border
    ]


def scenes():
    raw = synth.raw_scene(seed=0, height=48, width=64, points_per_view=40, frame_nums=[3, 7, 11])
    first = raw['sparse_depth_data'][3]
    for i, name in enumerate(COLUMNS):
        first[name] = numpy.concatenate([first[name], numpy.array([row[i] for row in planted_points(48, 64)])])
    del raw['sparse_depth_data'][7]
    yield 'ndc_sparse', configs(True, sparse_depth={'num_rays': 32}), raw

    raw = synth.raw_scene(seed=1, height=37, width=53, rgba=True, dense_dtype=numpy.float32, frame_nums=[0, 1, 2])
    del raw['sparse_depth_data']
    # float32 bounds: in world space the reference's near is bounds[0] * .9, and a float64 one makes its near / far cache columns
    # float64 under numpy 2 (NEP 50), which its own batch gather then refuses
    raw['nerf_data']['bounds'] = raw['nerf_data']['bounds'].astype(numpy.float32)
    yield 'world_dense', configs(False, white_bkgd=True, recenter_camera_poses=False, dense_depth={}), raw

    raw = synth.raw_scene(seed=2, height=24, width=32, points_per_view=25, dense_dtype=numpy.float64, frame_nums=[5, 6, 9])
    yield 'ndc_both', configs(True, bd_factor=None, sparse_depth={'num_rays': 16}, dense_depth={}, num_rays=64), raw


def for_reference(raw):
    """A deep copy in the loader's own types: the sparse tables as pandas DataFrames.  (The reference scales ``bounds`` in place.)"""
    out = copy.deepcopy(raw)
    if 'sparse_depth_data' in out:
        out['sparse_depth_data'] = {f: pandas.DataFrame(table) for f, table in out['sparse_depth_data'].items()}
    return out


def held_out_pose(seed):
    rng = numpy.random.RandomState(seed + 900)
    pose = numpy.eye(4)
    pose[:3, :3] = synth._rotation(*(0.05 * rng.standard_normal(3)))
    pose[:3, 3] = [0.3 * rng.standard_normal(), 0.2 * rng.standard_normal(), 0.1 * rng.standard_normal()]
    return pose


def main():
    for seed, (name, cfg, raw) in enumerate(scenes()):
        arrays = {'configs_json': numpy.array(json.dumps(cfg)), 'raw_frame_nums': numpy.asarray(raw['frame_nums'])}
        arrays.update({f'raw_{k}': numpy.asarray(v) for k, v in raw['nerf_data'].items()})
        for frame, table in raw.get('sparse_depth_data', {}).items():
            arrays.update({f'raw_sparse_{frame}_{k}': table[k] for k in COLUMNS})
        arrays.update({f'raw_dense_{k}': v for k, v in raw.get('dense_depth_data', {}).items()})
        if name == 'ndc_sparse':
            arrays['planted_names'] = numpy.array([row[4] for row in planted_points(48, 64)])

        numpy.random.seed(7 + seed)
        pp = DataPreprocessor(cfg, mode='train', raw_data_dict=for_reference(raw))
        data = pp.preprocessed_data_dict
        nerf = data['nerf_data']
        model_configs = pp.get_model_configs()
        arrays.update(poses=nerf['poses'], intrinsics=nerf['intrinsics'], images=nerf['images'].astype(numpy.float32),
                      sc=numpy.float64(nerf['sc']), average_pose=nerf['average_pose'], bounds=nerf['bounds'],
                      near=numpy.float64(nerf['near']), far=numpy.float64(nerf['far']),
                      model_configs_json=numpy.array(json.dumps(model_configs, default=float)))     # (float32 near / far: world scene)
        assert nerf['images'].dtype == numpy.float32
        if cfg['data_loader']['ndc']:
            arrays.update(near_ndc=numpy.float64(nerf['near_ndc']), far_ndc=numpy.float64(nerf['far_ndc']))
        if 'sparse_depth' in cfg['data_loader']:
            sd = data['sparse_depth_data']
            arrays.update(sparse_depths=sd['depths'].numpy().reshape(-1), sparse_errors=sd['reprojection_errors'].numpy().reshape(-1),
                          sparse_depths_ndc=sd['depths_ndc'].numpy().reshape(-1))
        if 'dense_depth' in cfg['data_loader']:
            dd = data['dense_depth_data']
            arrays.update(dense_depths=dd['depth_values'].numpy().reshape(-1), dense_depth_weights=dd['depth_weights'].numpy().reshape(-1))
            if cfg['data_loader']['ndc']:
                arrays['dense_depths_ndc'] = dd['depth_values_ndc'].numpy().reshape(-1)
        for b in range(3):
            batch = pp.get_next_batch(iter_num=b)
            for key, value in batch.items():
                if isinstance(value, torch.Tensor):
                    arrays[f'batch{b}_{key}'] = value.numpy()
                elif key != 'common_data':
                    arrays[f'batch{b}_{key}'] = numpy.asarray(value)

        # test mode, derived from what the train run saved: the training poses again, and a held-out pose as a full frame
        saved = json.loads(json.dumps(model_configs, default=float))
        tester = DataPreprocessor(cfg, mode='test', model_configs=saved)
        arrays['poses_test_mode'] = tester.preprocess_poses(
            {'poses': raw['nerf_data']['extrinsics'].copy(), 'translation_scale': saved['translation_scale'],
             'average_pose': numpy.array(saved['average_pose'])}, train_mode=False)['poses']
        pose = held_out_pose(seed)
        arrays['test_pose'] = pose
        for key, value in tester.create_test_data(pose).items():
            arrays[f'test_{key}'] = value.numpy()

        path = os.path.join(OUT, f'scene_prep_{name}.npz')
        numpy.savez_compressed(path, **arrays)
        print(f'{os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays; sc {nerf["sc"]!r} near '
              f'{nerf["near"]!r} far {nerf["far"]!r}')


if __name__ == '__main__':
    main()
