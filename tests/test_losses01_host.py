"""The plain (01) depth losses and dense-depth supervision, host side: what ``LossComputer`` accepts and refuses at
construction, the term count it derives from a configuration, the C ABI's new struct tail, and the fixtures' sizes."""
import copy
import ctypes
import os
import re

import numpy
import pytest

from simplenerf_amd import _lib, synth
from simplenerf_amd.loss_functions import LossComputer01
from simplenerf_amd.loss_functions.LossComputer01 import LossComputer
from tests import util

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('PointsAugmentationDepthLoss01', 'ViewsAugmentationDepthLoss01', 'CoarseFineConsistencyLoss01', 'DenseDepthMSE01')


def thirteen():
    return synth.loss_configs() + synth.loss_configs01(dense=True)[6:]


def shipped(kind='config3'):
    cfg = synth.make_configs(kind)
    cfg['data_loader']['sparse_depth'] = {}
    return cfg


@pytest.mark.parametrize('name', NEW)
def test_each_new_loss_constructs(name):
    cfg = shipped()
    cfg['losses'] = [{'name': name, 'weight': 0.1}]
    assert list(LossComputer(cfg).losses) == [name]
    assert name in LossComputer01.SUPPORTED


@pytest.mark.parametrize('name', ['VisibilityLoss01', 'VisibilityPriorLoss01'])
def test_the_visibility_losses_stay_refused(name):
    cfg = shipped()
    cfg['losses'] = [{'name': 'MSE01', 'weight': 1}, {'name': name, 'weight': 0.1}]
    with pytest.raises(RuntimeError, match='Unknown Loss Function'):
        LossComputer(cfg)
    assert len(LossComputer01.SUPPORTED) == 13


def test_all_thirteen_fill_the_table_exactly_on_the_shipped_model():
    cfg = shipped()
    cfg['losses'] = synth.loss_configs()
    assert sum(LossComputer01.term_capacity(cfg).values()) == 11
    cfg['losses'] = thirteen()
    capacity = LossComputer01.term_capacity(cfg)
    assert sum(capacity.values()) == 16 == LossComputer01.MAX_TERMS == _lib.LOSS_MAX_TERMS
    assert capacity['DenseDepthMSE01'] == 2 and capacity['CoarseFineConsistencyLoss01'] == 1
    assert capacity['CoarseFineConsistencyLoss02'] == 2 and capacity['PointsAugmentationDepthLoss01'] == 1
    assert len(LossComputer(cfg).losses) == 13


def test_a_list_that_cannot_fit_the_table_is_refused_at_construction_by_name():
    cfg = shipped('config3f')
    cfg['losses'] = synth.loss_configs()
    assert sum(LossComputer01.term_capacity(cfg).values()) == 15
    LossComputer(cfg)                                   # the nine shipped losses still fit with fine augmentation MLPs
    cfg['losses'] = thirteen()
    with pytest.raises(RuntimeError, match=r'16 terms.*can take 22') as error:
        LossComputer(cfg)
    for name in NEW + ('MSE02', 'CoarseFineConsistencyLoss02'):
        assert name in str(error.value)
    assert 'PointsAugmentationDepthLoss01 2' in str(error.value)


def test_term_counts_follow_the_model():
    cfg = shipped()
    del cfg['model']['fine_mlp']
    cfg['losses'] = thirteen()
    capacity = LossComputer01.term_capacity(cfg)
    assert capacity['CoarseFineConsistencyLoss01'] == 0 and capacity['CoarseFineConsistencyLoss02'] == 0
    assert capacity['DenseDepthMSE01'] == 1 and capacity['MSE01'] == 1 and capacity['PointsAugmentationDepthLoss02'] == 1
    no_sparse = synth.make_configs('config3')
    no_sparse['losses'] = thirteen()
    assert LossComputer01.term_capacity(no_sparse)['CoarseFineConsistencyLoss02'] == 1


def test_iter_weights_apply_to_the_new_losses():
    cfg = shipped()
    cfg['losses'] = synth.loss_configs01(dense=True)
    computer = LossComputer(cfg)
    late = computer.losses['CoarseFineConsistencyLoss01']
    assert computer.get_loss_weight(late, 0) == 0 and computer.get_loss_weight(late, 10000) == 0.1
    assert computer.get_loss_weight(computer.losses['DenseDepthMSE01'], 5) == 0.1


def test_abi_version_and_struct_tail():
    with open(os.path.join(REPO, 'include', 'simplenerf_hip.h')) as f:
        version = int(re.search(r'#define SNERF_ABI_VERSION (\d+)', f.read()).group(1))
    assert version == _lib.ABI_VERSION == 10
    names = [name for name, _ in _lib.LossTerm._fields_]
    assert names[-2:] == ['d_target', 'accumulate_target'] and names[:9] == [
        'pred', 'target', 'numerator_mask', 'denominator_mask', 'd_pred', 'channels', 'group', 'accumulate', 'weight']
    # the fields of ABI 9 keep their offsets: a caller that zero-initialises the struct and fills those gets a one-sided term
    assert _lib.LossTerm.weight.offset == 52 and _lib.LossTerm.d_target.offset == 56 and ctypes.sizeof(_lib.LossTerm) == 72
    with open(os.path.join(REPO, 'include', 'simplenerf_train.h')) as f:
        header = f.read()
    body = header[header.index('typedef struct snerf_loss_term'):header.index('} snerf_loss_term;')]
    assert body.index('float weight;') < body.index('float* d_target;') < body.index('int accumulate_target;')
    assert 'snerf_gather_dense_depth' in header and 'snerf_gather_dense_depth' in _lib.SIGNATURES


def test_fixture_sizes_and_contents():
    golden = os.path.join(REPO, 'tests', 'golden')
    limit = os.path.getsize(os.path.join(golden, 'losses_nosd.npz'))
    for case in synth.LOSS01_CASES:
        assert os.path.getsize(os.path.join(golden, f'losses01_{case}.npz')) <= limit, case
        g = util.load(f'losses01_{case}.npz')
        configs, _, batch, keys = synth.loss01_case(case)
        for cfg in configs['losses']:
            assert f"value_{cfg['name']}" in g, (case, cfg['name'])
        for k in keys:
            assert g[f'grad_{k}'].shape == batch[k].shape, (case, k)
    assert os.path.getsize(os.path.join(golden, 'batch_dense_depth.npz')) <= os.path.getsize(os.path.join(golden, 'batch_assembly.npz'))
    # the weight-0 case: the consistency losses have their value and move nothing
    early, world = util.load('losses01_early.npz'), util.load('losses01_world.npz')
    assert float(early['value_CoarseFineConsistencyLoss01']) == float(world['value_CoarseFineConsistencyLoss01']) > 0
    assert not early['grad_points_augmentation_depth_coarse'][:320].any() \
        and numpy.count_nonzero(world['grad_points_augmentation_depth_coarse']) > 300      # (a tenth of the rows are exact ties)
    # two-sided in the reference: depth_fine is read on the pixel rows by CoarseFineConsistencyLoss01 alone, as its target
    assert numpy.count_nonzero(world['grad_depth_fine'][:320]) == 320
    empty = util.load('losses01_empty.npz')
    assert float(empty['value_DenseDepthMSE01']) == 0.0 and float(empty['value_CoarseFineConsistencyLoss01']) > 0
    assert empty['map/DenseDepthMSE01/DenseDepthMSE01_coarse'].shape == (0,)


def test_dense_depth_column_follows_the_loader():
    scene = synth.synth_scene(0)
    tables = synth.dense_depth_tables(scene, 0)
    batch = synth.loss_batch(scene, 40, 8, 3)
    column = synth.dense_depth_column(batch, tables, scene)
    assert column.shape == (48, 1) and column.dtype == numpy.float32 and (column[40:] == -1).all()
    v, x, y = batch['pixel_id'][7]
    assert column[7, 0] == tables['dense_depths'].reshape(3, 48, 64)[v, y, x]
    assert (tables['dense_depths'] == -1).any() and (tables['dense_depths_ndc'][tables['dense_depths'] == -1] == -1).all()
    cfg = copy.deepcopy(synth.loss01_case('dense')[0])
    assert 'dense_depth' in cfg['data_loader'] and 'fine_mlp' not in cfg['model']
