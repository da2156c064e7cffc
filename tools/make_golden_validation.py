#!/usr/bin/env python3
"""Golden vectors for the validation mode and the trainer's validation pass, made by RUNNING THE REFERENCE on the CPU.

    SIMPLENERF_REFERENCE_SRC=<reference checkout>/src PYTHONDONTWRITEBYTECODE=1 python3 tools/make_golden_validation.py

One seeded 24x32 scene (``synth.raw_scene``, five views) is split into three training views and two held-out views with their own
frame numbers and their own ``bounds``.  skimage is stubbed as in tools/make_golden_scene.py; ``torch.utils.tensorboard``,
``deepdiff`` and ``simplejson`` are stubbed too: the trainer only logs and writes through them.

  validation_prep_ndc.npz     NDC, a ``sparse_depth`` loader section (train mode only: the held-out data carries no points)
  validation_prep_world.npz   world space, float32 bounds (tools/make_golden_scene.py says why), a ``dense_depth`` section
      the raw inputs of both splits, the reference's train-mode model configs (JSON), the validation-mode preprocessor's processed
      poses, bounds, near / far, float images and intrinsics, ``get_next_batch(0, frame)`` of both held-out frames (``val<frame>_*``)
      and of one training frame of the train-mode preprocessor (``train<frame>_*``), and each batch's key list
  validation_pass.npz         ``Trainer.run_validation`` (src/Trainer01.py:109-263) on the NDC scene over the validation and the
      train preprocessor (:302-305 runs both), on a ``Trainer`` made without its logger: a 4x128 coarse + fine MLP pair (64 + 128
      samples) with ``synth`` weights of seed 211, density heads calibrated as in tools/make_golden.py (stored: ``ovr_*``), fine MLP =
      coarse MLP; ``validation_chunk_size`` 200 (a 768-pixel frame is 3 chunks of 200 and one of 168);
      ``validation_save_loss_maps`` True.  The stubbed ``skimage.io.imsave`` and a patched ``numpy.save`` record every array the
      trainer writes: ``<val|train>/<directory>/<file stem>`` holds the float map (``.npy``), the same name with ``.png`` the uint8
      preview the reference computed from it; ``<val|train>_rgb/<file name>`` is the float colour frame ``save_image`` was handed for a
      colour PNG (it writes no ``.npy`` of it).  ``<val|train>_total_<loss>`` are the returned totals, ``<val|train>_acc_<level>_<frame>``
      the model's opacities of the frame (not written by the trainer; the tests' depth gates need them).

The loss list is MSE01 + CoarseFineConsistencyLoss01 -- of the losses this build has, the ones the reference completes in eval mode
over both preprocessors.  ``probe_losses`` below (``--probe``) runs each candidate alone and prints what the reference raises for the
others: SparseDepthMSE01 -- KeyError 'loss_maps' (its result has none and Trainer01.py:256 indexes them); CoarseFineConsistencyLoss02
-- completes over the training views, KeyError 'poses' over the held-out ones (their ``common_data`` is empty); the 02 / 03
augmentation losses -- their constructors need the model's augmentation sections, and with those the eval-mode model does not
produce the outputs they read (src/models/SimpleNeRF01.py:170, :186).
"""
import copy
import json
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy
import pandas
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.environ['SIMPLENERF_REFERENCE_SRC'])       # the src/ directory of a checkout of the reference
WRITTEN = {}                                                     # path relative to the save directory -> array


def _record(path, array, **kwargs):
    WRITTEN[os.fspath(path)] = numpy.array(array)


for name in ('skimage', 'skimage.io', 'skimage.transform', 'torch.utils.tensorboard', 'deepdiff', 'simplejson'):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules['skimage'].io = sys.modules['skimage.io']
sys.modules['skimage'].transform = sys.modules['skimage.transform']
sys.modules['skimage.io'].imsave = _record
sys.modules['torch.utils.tensorboard'].SummaryWriter = object
sys.modules['deepdiff'].DeepDiff = object

import Trainer01  # noqa: E402  (the reference)
from data_preprocessors.DataPreprocessor01 import DataPreprocessor  # noqa: E402
from loss_functions.LossComputer01 import LossComputer  # noqa: E402
from models.SimpleNeRF01 import SimpleNeRF  # noqa: E402

from simplenerf_amd import synth  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import calibrate_density, load_synth, tie_fine_to_coarse  # noqa: E402  (the helpers of the e2e fixtures)

OUT = os.path.join(REPO, 'tests', 'golden')
TRAIN_VIEWS, HELD_VIEWS = (0, 1, 2), (3, 4)
FRAME_NUMS = (2, 5, 8, 3, 6)
HELD_BOUNDS = (2.4, 6.2)
MODEL_SEED = 211
LOSSES = [{'name': 'MSE01', 'weight': 1}, {'name': 'CoarseFineConsistencyLoss01', 'weight': 0.1}]
CANDIDATES = ('MSE01', 'SparseDepthMSE01', 'CoarseFineConsistencyLoss01', 'CoarseFineConsistencyLoss02', 'MSE02',
              'PointsAugmentationDepthLoss02')


def configs(ndc, **loader):
    small = dict(depth=4, width=128, views_width=64)
    return {'data_loader': {'bd_factor': 0.75, 'batching': True, 'ndc': ndc, 'downsampling_factor': 1, 'num_rays': 96,
                            'recenter_camera_poses': True, 'spherify': False, 'precrop_iterations': 0, **loader},
            'model': {'name': 'SimpleNeRF01', 'chunk': 4096, 'lindisp': False, 'netchunk': 16384, 'perturb': True, 'raw_noise_std': 1.0,
                      'white_bkgd': False, 'coarse_mlp': synth.mlp_config(64, **small), 'fine_mlp': synth.mlp_config(128, **small)},
            'losses': copy.deepcopy(LOSSES), 'validation_chunk_size': 200, 'validation_save_loss_maps': True, 'device': 'cpu'}


def split(raw, views, bounds=None):
    """The loader's dictionary for some of the views of ``raw``."""
    views = list(views)
    nerf = raw['nerf_data']
    out = {'frame_nums': numpy.asarray(raw['frame_nums'])[views],
           'nerf_data': {'images': nerf['images'][views], 'extrinsics': nerf['extrinsics'][views], 'intrinsics': nerf['intrinsics'][views],
                         'bounds': numpy.array(nerf['bounds'] if bounds is None else bounds, dtype=nerf['bounds'].dtype),
                         'resolution': nerf['resolution']}}
    return out


def scenes():
    raw = synth.raw_scene(seed=5, num_views=5, height=24, width=32, points_per_view=25, frame_nums=FRAME_NUMS)
    train = split(raw, TRAIN_VIEWS)
    train['sparse_depth_data'] = {int(f): raw['sparse_depth_data'][int(f)] for f in train['frame_nums']}
    yield 'ndc', configs(True, sparse_depth={'num_rays': 16}), train, split(raw, HELD_VIEWS, HELD_BOUNDS)

    raw = synth.raw_scene(seed=6, num_views=5, height=24, width=32, dense_dtype=numpy.float32, frame_nums=FRAME_NUMS)
    raw['nerf_data']['bounds'] = raw['nerf_data']['bounds'].astype(numpy.float32)
    train = split(raw, TRAIN_VIEWS)
    train['dense_depth_data'] = {k: v[list(TRAIN_VIEWS)] for k, v in raw['dense_depth_data'].items()}
    yield 'world', configs(False, dense_depth={}), train, split(raw, HELD_VIEWS, HELD_BOUNDS)


def for_reference(raw):
    """A deep copy in the loader's own types: the sparse tables as pandas DataFrames.  (The reference scales ``bounds`` in place.)"""
    out = copy.deepcopy(raw)
    if 'sparse_depth_data' in out:
        out['sparse_depth_data'] = {f: pandas.DataFrame(table) for f, table in out['sparse_depth_data'].items()}
    return out


def preprocessors(cfg, train_raw, held_raw):
    numpy.random.seed(31)
    train = DataPreprocessor(cfg, mode='train', raw_data_dict=for_reference(train_raw))
    held = DataPreprocessor(cfg, mode='validation', raw_data_dict=for_reference(held_raw), model_configs=train.get_model_configs())
    return train, held


def batch_arrays(prefix, batch):
    arrays = {f'{prefix}_keys': numpy.array(sorted(batch.keys())), f'{prefix}_common_data_keys': numpy.array(sorted(batch['common_data']))}
    for key, value in batch.items():
        if key != 'common_data':
            arrays[f'{prefix}_{key}'] = value.numpy() if isinstance(value, torch.Tensor) else numpy.asarray(value)
    return arrays


def make_prep(name, cfg, train_raw, held_raw):
    arrays = {'configs_json': numpy.array(json.dumps(cfg))}
    for tag, raw in (('train', train_raw), ('val', held_raw)):
        arrays[f'raw_{tag}_frame_nums'] = numpy.asarray(raw['frame_nums'])
        arrays.update({f'raw_{tag}_{k}': numpy.asarray(v) for k, v in raw['nerf_data'].items()})
        for frame, table in raw.get('sparse_depth_data', {}).items():
            arrays.update({f'raw_{tag}_sparse_{frame}_{k}': table[k] for k in ('x', 'y', 'depth', 'reprojection_error')})
        arrays.update({f'raw_{tag}_dense_{k}': v for k, v in raw.get('dense_depth_data', {}).items()})
    train, held = preprocessors(cfg, train_raw, held_raw)
    arrays['model_configs_json'] = numpy.array(json.dumps(train.get_model_configs(), default=float))
    assert held.get_model_configs() is train.get_model_configs()
    nerf = held.preprocessed_data_dict['nerf_data']
    assert nerf['images'].dtype == numpy.float32 and nerf['intrinsics'].dtype == numpy.float32
    assert 'sparse_depth_data' not in held.preprocessed_data_dict and 'dense_depth_data' not in held.preprocessed_data_dict
    arrays.update(val_poses=nerf['poses'], val_bounds=nerf['bounds'], val_near=numpy.float64(nerf['near']), val_far=numpy.float64(nerf['far']),
                  val_images=nerf['images'], val_intrinsics=nerf['intrinsics'])
    if cfg['data_loader']['ndc']:
        arrays.update(val_near_ndc=numpy.float64(nerf['near_ndc']), val_far_ndc=numpy.float64(nerf['far_ndc']))
    for frame in held_raw['frame_nums'].tolist():
        arrays.update(batch_arrays(f'val{frame}', held.get_next_batch(0, frame)))
    frame = int(train_raw['frame_nums'][1])
    arrays.update(batch_arrays(f'train{frame}', train.get_next_batch(0, frame)))
    path = os.path.join(OUT, f'validation_prep_{name}.npz')
    numpy.savez_compressed(path, **arrays)
    print(f'{os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays; validation near {nerf["near"]!r} far '
          f'{nerf["far"]!r} against the training scene\'s {train.preprocessed_data_dict["nerf_data"]["near"]!r} '
          f'{train.preprocessed_data_dict["nerf_data"]["far"]!r}')


def trainer_for(cfg, train, held):
    """A Trainer without its logger (the constructor opens a SummaryWriter) and the model's calibrated density heads."""
    model = load_synth(SimpleNeRF(cfg, train.get_model_configs()), MODEL_SEED)
    model.eval()
    batch = train.get_next_batch(0, int(train.preprocessed_data_dict['frame_nums'][0]))
    overrides = {k: v for k, v in calibrate_density(model, batch, train_mode=False).items() if not k.startswith('ovr_fine_model')}
    overrides.update(tie_fine_to_coarse(model))
    trainer = Trainer01.Trainer.__new__(Trainer01.Trainer)
    trainer.configs, trainer.model_configs = cfg, train.get_model_configs()
    trainer.train_data_loader, trainer.val_data_loader = train, held
    trainer.model, trainer.loss_computer = model, LossComputer(cfg)
    trainer.device = torch.device('cpu')
    return trainer, overrides


def recorded_validation(trainer, iter_num, loader, tag):
    """-> (the totals, {'<tag>/<directory>/<file name>': array}): the trainer only makes its (empty) directories, in a temporary place."""
    save, save_image = numpy.save, Trainer01.Trainer.save_image
    colours = {}

    def recording_save_image(path, image):
        colours[path.as_posix()] = numpy.array(image)          # the float colour frame save_image converts (:387)
        return save_image(path, image)

    numpy.save, Trainer01.Trainer.save_image = _record, staticmethod(recording_save_image)
    WRITTEN.clear()
    try:
        with tempfile.TemporaryDirectory() as tmp:
            totals = trainer.run_validation(iter_num, loader, Path(tmp) / tag)
            written = {os.path.relpath(path, tmp): array for path, array in WRITTEN.items()}
            written.update({f'{tag}_rgb/' + os.path.relpath(path, os.path.join(tmp, tag)): array for path, array in colours.items()})
    finally:
        numpy.save, Trainer01.Trainer.save_image = save, staticmethod(save_image)
    return totals, written


def make_pass(cfg, train_raw, held_raw):
    train, held = preprocessors(cfg, train_raw, held_raw)
    trainer, overrides = trainer_for(cfg, train, held)
    arrays = {'seed': MODEL_SEED, 'iter_num': 41, 'losses_json': numpy.array(json.dumps(cfg['losses']))}
    arrays.update({k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in overrides.items()})
    for tag, loader in (('val', held), ('train', train)):
        totals, written = recorded_validation(trainer, 41, loader, tag)
        assert trainer.model.training
        for name, value in totals.items():
            arrays[f'{tag}_total_{name}'] = numpy.float64(value)
        arrays.update(written)
        # the opacities, which the trainer does not write: the depth gates of the tests hold on rays with acc > 1e-2 only
        trainer.model.eval()
        for frame in loader.preprocessed_data_dict['frame_nums'].tolist():
            with torch.no_grad():
                out = trainer.model(loader.get_next_batch(41, frame))
            arrays.update({f'{tag}_acc_{level}_{frame}': out[f'acc_{level}'].numpy() for level in ('coarse', 'fine')})
        trainer.model.train()
        print(f'   {tag}: {len(written)} arrays written, totals {totals}')
    path = os.path.join(OUT, 'validation_pass.npz')
    numpy.savez_compressed(path, **arrays)
    print(f'{os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays')


def probe_losses(cfg, train_raw, held_raw):
    """Which of the losses this build has does the reference's validation pass complete?  One loss at a time, both preprocessors."""
    for name in CANDIDATES:
        one = copy.deepcopy(cfg)
        one['losses'] = [{'name': name, 'weight': 1, 'rmse_threshold': 0.1, 'patch_size': [5, 5]}]
        train, held = preprocessors(one, train_raw, held_raw)
        for tag, loader in (('val', held), ('train', train)):
            try:
                trainer, _ = trainer_for(one, train, held)
                recorded_validation(trainer, 0, loader, tag)
                print(f'{name} / {tag}: completes')
            except Exception as error:  # noqa: BLE001  (the point is to see what the reference raises)
                print(f'{name} / {tag}: {type(error).__name__}: {error}')


def main():
    made = list(scenes())
    if '--probe' in sys.argv:
        probe_losses(*made[0][1:])
        return
    for name, cfg, train_raw, held_raw in made:
        make_prep(name, cfg, train_raw, held_raw)
    make_pass(*made[0][1:])


if __name__ == '__main__':
    main()
