"""CPU-only checks of the validation mode and the validation pass: the host-side preparation of a validation-mode DataPreprocessor
against the fixtures made by running the reference (tools/make_golden_validation.py), the host view both modes expose to a trainer,
the chunk merge rule on hand-made dictionaries, the PNG decoder the GPU tests rely on, and the new C-ABI symbol."""
import ctypes
import json
import os
import re

import numpy
import pytest
import torch

from simplenerf_amd import _lib, harness, ops
from simplenerf_amd.data_preprocessors import DataPreprocessor01 as dp
from tests import util
from tests import validation_reference as ref
from tests.test_scene_host import ulps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', params=ref.CASES)
def case(request):
    return (request.param,) + ref.load_prep(request.param)


# ------------------------------------------------------------------------------------------------ host-side preparation
def test_validation_pose_preparation_equals_the_reference(case):
    """The gates of tests/test_scene_host.py for the train mode: one fp32 ulp on poses, 1e-12 relative on scalars."""
    name, g, configs, train_raw, held_raw = case
    saved = ref.model_configs(g)
    host = dp.prepare_host(configs, held_raw, 'validation', saved)
    assert host['poses'].dtype == numpy.float32 and host['poses'].shape == g['val_poses'].shape == (2, 4, 4)
    distance = ulps(host['poses'], g['val_poses'])
    util.observe(f'validation poses {name}', f'{distance} ulp from the reference [1]')
    assert distance <= 1, distance
    rel = lambda a, b: float(numpy.max(numpy.abs(numpy.asarray(a, dtype=numpy.float64) - b) / numpy.maximum(numpy.abs(b), 1e-300)))
    figures = {'near': rel(host['near'], g['val_near']), 'far': rel(host['far'], g['val_far']), 'bounds': rel(host['bounds'], g['val_bounds'])}
    util.observe(f'validation scalars {name}', f'{figures} [1e-12 relative]')
    assert all(v <= 1e-12 for v in figures.values()), figures
    assert numpy.array_equal(host['intrinsics'], g['val_intrinsics']) and host['intrinsics'].dtype == numpy.float32
    assert numpy.array_equal(host['average_pose'], numpy.array(saved['average_pose']))
    assert 'sc' not in host and 'points' not in host           # no scale of its own, no sparse-depth points: train mode only
    if configs['data_loader']['ndc']:
        assert (host['near_ndc'], host['far_ndc']) == (float(g['val_near_ndc']), float(g['val_far_ndc'])) == (0.0, 1.0)
    # the held-out views' own bounds, scaled by the TRAINING scene's factor: not the training scene's near / far
    assert not numpy.isclose(host['near'], saved['near']) and not numpy.isclose(host['far'], saved['far'])
    expected = numpy.asarray(held_raw['nerf_data']['bounds'], dtype=numpy.float64) * saved['translation_scale']
    assert numpy.allclose(host['bounds'], expected, rtol=1e-6)
    assert numpy.array_equal(held_raw['nerf_data']['bounds'], g['raw_val_bounds'])           # the caller's array is not scaled in place


def test_the_held_out_views_are_not_the_training_views(case):
    name, g, configs, train_raw, held_raw = case
    assert not set(train_raw['frame_nums'].tolist()) & set(held_raw['frame_nums'].tolist())
    assert len(train_raw['frame_nums']) == 3 and len(held_raw['frame_nums']) == 2
    assert 'sparse_depth_data' not in held_raw and 'dense_depth_data' not in held_raw
    loader = configs['data_loader']
    assert ('sparse_depth' in loader) == (name == 'ndc') and ('dense_depth' in loader) == (name == 'world')


@pytest.mark.parametrize('mode', ['train', 'validation'])
def test_host_view_has_what_a_trainer_reads(case, mode):
    name, g, configs, train_raw, held_raw = case
    raw = train_raw if mode == 'train' else held_raw
    host = dp.prepare_host(configs, raw, mode, None if mode == 'train' else ref.model_configs(g))
    view = dp.host_view(host, configs['data_loader']['ndc'])
    assert set(view) == {'frame_nums', 'nerf_data'}
    assert isinstance(view['frame_nums'], numpy.ndarray) and numpy.issubdtype(view['frame_nums'].dtype, numpy.integer)
    assert view['frame_nums'].tolist() == raw['frame_nums'].tolist()
    nerf = view['nerf_data']
    names = {'resolution', 'poses', 'intrinsics', 'bounds', 'near', 'far', 'average_pose'}
    names |= {'near_ndc', 'far_ndc'} if configs['data_loader']['ndc'] else set()
    names |= {'sc'} if mode == 'train' else set()
    assert set(nerf) == names
    views = len(raw['frame_nums'])
    assert nerf['resolution'] == [24, 32] and all(isinstance(x, int) for x in nerf['resolution'])
    assert isinstance(nerf['poses'], numpy.ndarray) and nerf['poses'].dtype == numpy.float32 and nerf['poses'].shape == (views, 4, 4)
    assert nerf['intrinsics'].dtype == numpy.float32 and nerf['intrinsics'].shape == (views, 3, 3)
    assert nerf['bounds'].shape == (2,) and nerf['average_pose'].shape == (4, 4)
    assert all(isinstance(nerf[k], float) for k in ('near', 'far'))
    for value in nerf.values():                        # nothing per pixel
        assert numpy.size(value) <= views * 16
    for frame_num in view['frame_nums']:               # the reference formats them with ':04' (src/Trainer01.py:234)
        assert f'{frame_num:04}' == '%04d' % int(frame_num)


def test_validation_mode_needs_the_training_model_configs():
    g, configs, train_raw, held_raw = ref.load_prep('ndc')
    with pytest.raises(RuntimeError, match='get_model_configs'):
        dp.DataPreprocessor(configs, 'validation', held_raw, device='cuda:0')
    bad = json.loads(json.dumps(configs))
    bad['data_loader']['spherify'] = True
    with pytest.raises(NotImplementedError, match='spherify'):
        dp.DataPreprocessor(bad, 'validation', held_raw, ref.model_configs(g), device='cuda:0')


# ------------------------------------------------------------------------------------------------ the chunk merge rule
def test_merge_concatenates_tensors_and_averages_scalars_chunk_by_chunk():
    sizes = (200, 200, 200, 168)            # a 768-pixel frame in chunks of 200: the last one is short
    rng = numpy.random.RandomState(3)
    chunks, values = [], []
    for size in sizes:
        value = float(rng.uniform())
        values.append(value)
        chunks.append({'rgb_fine': torch.from_numpy(rng.uniform(size=(size, 3)).astype(numpy.float32)),
                       'depth_fine': torch.from_numpy(rng.uniform(size=(size,)).astype(numpy.float32)),
                       'TotalLoss': torch.tensor(value, dtype=torch.float64)})
    merged = harness.merge_chunks(chunks)
    assert list(merged) == ['rgb_fine', 'depth_fine', 'TotalLoss']
    assert merged['rgb_fine'].shape == (768, 3) and merged['depth_fine'].shape == (768,)
    assert torch.equal(merged['rgb_fine'][600:], chunks[3]['rgb_fine']) and torch.equal(merged['depth_fine'][200:400], chunks[1]['depth_fine'])
    # the PLAIN mean of the chunk values: the short chunk weighs as much as a full one (src/Trainer01.py:153)
    plain = sum(values) / 4
    weighted = sum(v * s for v, s in zip(values, sizes)) / 768
    assert abs(float(merged['TotalLoss']) - plain) <= 1e-15 and abs(plain - weighted) > 1e-4
    assert merged['TotalLoss'].dim() == 0


def test_merge_handles_the_nested_loss_dictionaries():
    def chunk(size, value, seed):
        maps = torch.from_numpy(numpy.random.RandomState(seed).uniform(size=(size,)).astype(numpy.float32))
        return {'MSE01': {'loss_value': torch.tensor(value), 'loss_maps': {'MSE01_coarse': maps, 'MSE01_fine': maps * 2}},
                'TotalLoss': torch.tensor(value * 3)}
    chunks = [chunk(5, 1.0, 0), chunk(5, 2.0, 1), chunk(2, 6.0, 2)]
    merged = harness.merge_chunks(chunks)
    assert float(merged['MSE01']['loss_value']) == 3.0 and float(merged['TotalLoss']) == 9.0
    assert merged['MSE01']['loss_maps']['MSE01_coarse'].shape == (12,)
    assert torch.equal(merged['MSE01']['loss_maps']['MSE01_fine'][10:], chunks[2]['MSE01']['loss_maps']['MSE01_fine'])
    # a single chunk merges to itself; what the reference's rule has no branch for raises, as there (:167-171)
    alone = harness.merge_chunks(chunks[:1])
    assert float(alone['TotalLoss']) == 3.0 and torch.equal(alone['MSE01']['loss_maps']['MSE01_coarse'], chunks[0]['MSE01']['loss_maps']['MSE01_coarse'])
    with pytest.raises(RuntimeError, match='merge_chunks'):
        harness.merge_chunks([{'num_frames': 3}])
    with pytest.raises(RuntimeError, match='merge_chunks'):
        harness.merge_chunks([{'MSE01': {'loss_value': torch.zeros(4)}}])


def test_divide_batch_slices_rows_and_copies_common_data():
    n = 7
    common = {'poses': torch.zeros(1, 3, 4, 4), 'resolution': (2, 4)}
    batch = {'rays_o': torch.arange(n * 3.).reshape(n, 3), 'indices': numpy.arange(n), 'iter_num': 4, 'num_frames': 3,
             'common_data': common, 'poses_like': torch.zeros(3, 4)}
    chunks = harness.divide_batch(batch, 3)
    assert [c['rays_o'].shape[0] for c in chunks] == [3, 3, 1] and chunks[2]['indices'].tolist() == [6]
    assert all(c['iter_num'] == 4 and c['poses_like'] is batch['poses_like'] for c in chunks)
    assert all(c['common_data'] == common and c['common_data'] is not common for c in chunks)


def test_the_dropped_keys_are_the_references():
    dropped = set(harness.VALIDATION_DROPPED_KEYS)
    assert len(dropped) == len(harness.VALIDATION_DROPPED_KEYS) == 54
    assert {'z_vals_coarse', 'raw_sigma_fine', 'alpha_fine', 'weights_coarse', 'visibility_fine', 'raw_rgb_view_dependent_coarse'} <= dropped
    assert not dropped & {'rgb_coarse', 'rgb_fine', 'acc_fine', 'depth_fine', 'depth_var_ndc_coarse', 'visibility2_fine'}


# ------------------------------------------------------------------------------------------------ the fixtures themselves
def test_the_reference_previews_are_the_numpy_expressions_of_its_float_maps():
    """The fixture is self-consistent: every recorded PNG is the conversion of the recorded float map beside it, and no map of it is
    degenerate (a maximum that is not positive and finite would make the reference's own cast undefined)."""
    g = util.load('validation_pass.npz')
    for tag, frames in (('val', 2), ('train', 3)):
        files = ref.written(g, tag)
        assert len(files) == frames * 24
        for name, array in files.items():
            if name.endswith('.npy'):
                assert array.dtype == numpy.float32 and array.shape == (24, 32)
                assert numpy.isfinite(array).all() and array.max() > 0
                assert numpy.array_equal(files[name[:-4] + '.png'], ref.preview_u8(array)), name
            else:
                assert array.dtype == numpy.uint8 and array.shape in ((24, 32), (24, 32, 3))
    assert len(files) == len({os.path.splitext(name)[0] for name in files}) + 3 * 11      # per frame: 11 float maps, each with a preview, and 2 colour frames


def test_png_decoder_inverts_the_writer():
    rng = numpy.random.RandomState(0)
    for shape in ((5, 7), (5, 7, 3), (1, 1), (24, 32, 3)):
        image = rng.randint(0, 256, size=shape).astype(numpy.uint8)
        assert numpy.array_equal(ref.decode_png(harness._png_bytes(image)), image)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_entry_point_is_declared_bound_and_exported():
    """The prototypes of the two headers under include/ are a pinned set (tests/test_cdecl_host.py, tests/test_host_logic.py), so
    the new entry point is declared in a header of its own beside the kernels, which the binding reads after them."""
    assert [os.path.relpath(path, REPO) for path in _lib.ADDED_HEADERS] == [os.path.join('simplenerf_amd', 'csrc', 'simplenerf_maps.h')]
    header = open(_lib.ADDED_HEADERS[0]).read()
    declared = set(re.findall(r'\b(snerf_[a-z_0-9]+)\s*\(', header))
    assert declared == set(_lib.ADDED_SIGNATURES) == {'snerf_maps_to_u8', 'snerf_maps_to_u8_workspace_bytes'}
    assert not set(_lib.ADDED_SIGNATURES) & set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.ADDED_SIGNATURES[name][1], name
    assert 'snerf_maps_to_u8' in open(os.path.join(REPO, 'include', 'simplenerf_hip.h')).read()          # (it says where to look)
    assert lib.snerf_abi_version() == _lib.ABI_VERSION == 10
    assert callable(ops.maps_to_u8) and (ops.MAP_SCALE_255, ops.MAP_SCALE_MAX) == (0, 1)
    restype, argtypes = _lib.ADDED_SIGNATURES['snerf_maps_to_u8']
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.snerf_maps_to_u8_workspace_bytes(0) == 0 and lib.snerf_maps_to_u8_workspace_bytes(-3) == 0
    assert lib.snerf_maps_to_u8_workspace_bytes(10) >= 10 * 4 and lib.snerf_maps_to_u8_workspace_bytes(10) % 4 == 0


def test_bad_arguments_are_refused_and_empty_calls_succeed_without_a_device():
    """Every check comes before the first launch, and an empty call launches nothing: both run with no GPU."""
    lib = _lib.load()
    one, null = ctypes.c_void_p(16), ctypes.c_void_p(0)          # never dereferenced
    message = lambda: lib.snerf_last_error().decode()
    assert lib.snerf_maps_to_u8(null, null, 0, 100, null, null, null, null) == 0           # K == 0
    assert lib.snerf_maps_to_u8(null, null, 4, 0, null, null, null, null) == 0             # n == 0
    for args, word in (((null, one, 2, 8, one, one, one), 'NULL'), ((one, null, 2, 8, one, one, one), 'NULL'),
                       ((one, one, 2, 8, null, one, one), 'NULL'), ((one, one, 2, 8, one, null, one), 'NULL'),
                       ((one, one, 2, 8, one, one, null), 'NULL'), ((one, one, -1, 8, one, one, one), 'num_maps'),
                       ((one, one, 65536, 8, one, one, one), 'num_maps'), ((one, one, 2, -8, one, one, one), 'negative'),
                       ((ctypes.c_void_p(18), one, 2, 8, one, one, one), 'aligned')):
        assert lib.snerf_maps_to_u8(*args, null) < 0 and word in message(), (args, message())
