"""CPU-only checks of the scene stage (raw loader data -> the scene of BatchAssembler): the numpy restatement of the kernels
(tests/scene_reference.py) against the fixtures made by running the reference's DataPreprocessor (tools/make_golden_scene.py), the
host-side pose preparation and model configs against the same fixtures, the refusals, and the new C-ABI symbols."""
import copy
import json
import os
import re

import numpy
import pytest

from simplenerf_amd import _lib, ops
from simplenerf_amd.data_preprocessors import DataPreprocessor01 as dp
from simplenerf_amd.data_preprocessors.DataPreprocessorFactory import get_data_preprocessor
from tests import scene_reference as ref
from tests import util

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('snerf_scene_images', 'snerf_rasterise_sparse_depth', 'snerf_rasterise_sparse_depth_workspace_bytes',
               'snerf_depth_table_to_ndc')


def same_bits(a, b):
    a, b = numpy.asarray(a), numpy.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == numpy.float32 and numpy.array_equal(ref.bits(a), ref.bits(b))


@pytest.fixture(scope='module', params=ref.CASES)
def case(request):
    g, configs, raw = ref.load_case(request.param)
    return request.param, g, configs, raw


# ------------------------------------------------------------------------------------------------ the restatement vs the reference
def test_restated_images_equal_the_reference(case):
    name, g, configs, raw = case
    assert same_bits(ref.prepare_images(raw['nerf_data']['images'], configs['model']['white_bkgd']), g['images'])
    if name == 'world_dense':       # RGBA on white: the composition really ran
        assert raw['nerf_data']['images'].shape[-1] == 4 and configs['model']['white_bkgd']


@pytest.mark.parametrize('name', ref.SPARSE_CASES)
def test_restated_sparse_tables_equal_the_reference(name):
    g, configs, raw = ref.load_case(name)
    h, w = raw['nerf_data']['resolution']
    p = dp.collect_points(raw)
    depths, errors = ref.rasterise(p['x'], p['y'], p['depth'], p['reprojection_error'], p['view'], 3, h, w, scale=float(g['sc']))
    assert same_bits(depths, g['sparse_depths']) and same_bits(errors, g['sparse_errors'])
    oz, dz = ref.pixel_rays_z(g['intrinsics'], g['poses'], h, w)
    assert same_bits(ref.depth_to_ndc(depths, oz, dz, 1), g['sparse_depths_ndc'])       # near plane 1, whatever the scene's


@pytest.mark.parametrize('name', ref.DENSE_CASES)
def test_restated_dense_tables_equal_the_reference(name):
    g, configs, raw = ref.load_case(name)
    h, w = raw['nerf_data']['resolution']
    sc = float(g['sc']) if configs['data_loader']['bd_factor'] is not None else 1
    values = raw['dense_depth_data']['depth_values']
    depths = (values * sc).astype(numpy.float32).reshape(-1)
    assert same_bits(depths, g['dense_depths'])
    assert same_bits(raw['dense_depth_data']['depth_weights'].astype(numpy.float32).reshape(-1), g['dense_depth_weights'])
    assert (values == -1).any()
    if configs['data_loader']['ndc']:
        oz, dz = ref.pixel_rays_z(g['intrinsics'], g['poses'], h, w)
        ndc = ref.depth_to_ndc(depths, oz, dz, float(g['near']))
        assert same_bits(ndc, g['dense_depths_ndc'])
        assert (depths == -1).any() and (ndc[depths == -1] == -1).all()


def test_planted_points_land_where_the_rules_say():
    """Duplicates, half-way coordinates, clipped points and the missing frame of scene_prep_ndc_sparse, one by one."""
    g, configs, raw = ref.load_case('ndc_sparse')
    h, w = raw['nerf_data']['resolution']
    sc = float(g['sc'])
    table = g['sparse_depths'].reshape(3, h, w)
    errors = g['sparse_errors'].reshape(3, h, w)
    value = lambda d: numpy.float32(d * sc)
    assert list(g['planted_names'][:2]) == ['repeat_first', 'repeat_last']
    assert table[0, 5, 10] == value(4.5) and errors[0, 5, 10] == numpy.float32(0.7)      # an exact repeat: the later point stays
    assert table[0, 7, 20] == value(3.3)                                                 # three points on one pixel: the last
    assert table[0, 12, 2] == value(3.4) and table[0, 13, 4] == value(3.5)               # 2.5 -> 2 and 3.5 -> 4: half to even
    assert table[0, 12, 3] == -1
    assert table[0, 0, 30] == value(3.6) and table[0, 0, 31] == value(3.7)               # rows 0.5 and -0.5 -> 0
    assert table[0, 20, 0] == value(3.8) and table[0, 21, w - 1] == value(3.9)           # left and right of the frame
    assert table[0, 0, 40] == value(4.0) and table[0, h - 1, 41] == value(4.1)           # above and below
    assert list(raw['frame_nums']) == [3, 7, 11] and 7 not in raw['sparse_depth_data']
    assert (table[1] == -1).all() and (errors[1] == -1).all() and (g['sparse_depths_ndc'].reshape(3, h, w)[1] == -1).all()
    assert (table[0] > 0).sum() > 40 and (table[2] > 0).sum() > 30


# ------------------------------------------------------------------------------------------------ pose preparation, model configs
def ulps(a, b):
    a, b = ref.bits(a).astype(numpy.int64), ref.bits(b).astype(numpy.int64)
    key = lambda u: numpy.where(u & 0x80000000, 0x80000000 - u, u)         # sign-magnitude -> a monotone integer line
    return int(numpy.abs(key(a) - key(b)).max())


def test_pose_preparation_equals_the_reference(case):
    name, g, configs, raw = case
    host = dp.prepare_host(configs, raw)
    saved = json.loads(str(g['model_configs_json']))
    test_mode = dp.prepare_poses(raw['nerf_data']['extrinsics'], train_mode=False, translation_scale=saved['translation_scale'],
                                 average_pose=saved['average_pose'])['poses']
    for tag, mine, theirs in (('train', host['poses'], g['poses']), ('test', test_mode, g['poses_test_mode'])):
        assert mine.dtype == numpy.float32 and mine.shape == theirs.shape
        distance = ulps(mine, theirs)
        util.observe(f'scene poses {name} {tag}', f'{distance} ulp from the reference [1]')
        assert distance <= 1, (tag, distance)
    rel = lambda a, b: float(numpy.max(numpy.abs(numpy.asarray(a, dtype=numpy.float64) - b) / numpy.maximum(numpy.abs(b), 1e-300)))
    figures = {'sc': rel(host['sc'], g['sc']), 'near': rel(host['near'], g['near']), 'far': rel(host['far'], g['far']),
               'average_pose': float(numpy.max(numpy.abs(host['average_pose'] - g['average_pose']))) / float(numpy.abs(g['average_pose']).max())}
    util.observe(f'scene scalars {name}', f'{figures} [1e-12 relative]')
    assert all(v <= 1e-12 for v in figures.values()), figures
    assert numpy.array_equal(host['intrinsics'], g['intrinsics']) and host['intrinsics'].dtype == numpy.float32
    assert numpy.allclose(host['bounds'], g['bounds'], rtol=1e-12, atol=0)
    if configs['data_loader']['ndc']:
        assert (host['near_ndc'], host['far_ndc']) == (float(g['near_ndc']), float(g['far_ndc'])) == (0.0, 1.0)
    if name == 'world_dense':
        assert numpy.array_equal(host['average_pose'], numpy.eye(4))         # recenter_camera_poses: False
    if name == 'ndc_both':
        assert host['sc'] == 1 and isinstance(host['sc'], int)                # bd_factor: None


def test_model_configs_are_the_references(case):
    name, g, configs, raw = case
    mine = dp.create_model_configs(dp.prepare_host(configs, raw), configs['data_loader']['ndc'])
    theirs = json.loads(str(g['model_configs_json']))
    assert json.loads(json.dumps(mine)).keys() == theirs.keys()              # and JSON-serialisable as it stands
    assert list(mine) == list(theirs)
    for key in ('resolution', 'train_frame_nums', 'intrinsic', 'translation_scale'):
        assert mine[key] == theirs[key], key
    for key in ('bounds', 'average_pose', 'near', 'far') + (('near_ndc', 'far_ndc') if 'near_ndc' in theirs else ()):
        assert numpy.allclose(numpy.array(mine[key], dtype=numpy.float64), numpy.array(theirs[key]), rtol=1e-12, atol=1e-15), key
    assert ('near_ndc' in mine) == bool(configs['data_loader']['ndc'])


def test_the_callers_arrays_come_back_unmodified(case):
    name, g, configs, raw = case
    before = copy.deepcopy(raw)
    host = dp.prepare_host(configs, raw)
    dp.create_model_configs(host, configs['data_loader']['ndc'])
    pose = g['test_pose'].copy()
    dp.prepare_poses(pose[None], train_mode=False, translation_scale=0.5, average_pose=numpy.eye(4))
    assert numpy.array_equal(pose, g['test_pose'])

    def same(a, b):
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        return numpy.array_equal(numpy.asarray(a), numpy.asarray(b)) and numpy.asarray(a).dtype == numpy.asarray(b).dtype
    assert same(raw, before)
    if configs['data_loader']['bd_factor'] is not None:
        assert not numpy.array_equal(host['bounds'], raw['nerf_data']['bounds'])         # (the reference scales them in place)


# ------------------------------------------------------------------------------------------------ refusals
def with_loader(configs, **loader):
    out = copy.deepcopy(configs)
    out['data_loader'].update(loader)
    return out


@pytest.mark.parametrize('loader, word', [({'downsampling_factor': 2}, 'downsampling_factor'), ({'spherify': True}, 'spherify'),
                                          ({'visibility_prior': {'load_masks': True, 'load_weights': False}}, 'visibility_prior'),
                                          ({'batching': False}, 'batching')])
def test_unbuilt_options_are_refused_by_name(loader, word):
    g, configs, raw = ref.load_case('ndc_sparse')
    for mode, kw in (('train', {'raw_data_dict': raw}), ('test', {'model_configs': json.loads(str(g['model_configs_json']))})):
        with pytest.raises(NotImplementedError, match=word):
            dp.DataPreprocessor(with_loader(configs, **loader), mode, **kw)


def test_other_cameras_view_directions_are_refused():
    g, configs, raw = ref.load_case('ndc_sparse')
    tester = get_data_preprocessor(with_loader(configs, data_preprocessor_name='DataPreprocessor01'), 'test',
                                   model_configs=json.loads(str(g['model_configs_json'])))
    assert isinstance(tester, dp.DataPreprocessor) and tester.get_model_configs()['resolution'] == [48, 64]
    with pytest.raises(NotImplementedError, match='view_pose'):
        tester.create_test_data(g['test_pose'], view_pose=g['test_pose'])
    with pytest.raises(NotImplementedError, match='secondary_poses'):
        tester.create_test_data(g['test_pose'], secondary_poses=[g['test_pose']])
    with pytest.raises(RuntimeError, match='Unknown data preprocessor'):
        get_data_preprocessor(with_loader(configs, data_preprocessor_name='NoSuchPreprocessor01'), 'test')


@pytest.mark.parametrize('bad', [numpy.nan, numpy.inf, -numpy.inf])
def test_non_finite_point_coordinates_are_refused(bad):
    g, configs, raw = ref.load_case('ndc_sparse')
    for column in ('x', 'y'):
        broken = copy.deepcopy(raw)
        broken['sparse_depth_data'][11][column][4] = bad
        with pytest.raises(ValueError, match='non-finite'):
            dp.DataPreprocessor(configs, 'train', broken, device='cuda:0')       # refused on the host, before any device work
        arrays = dp.collect_points(raw)
        arrays[column] = arrays[column].copy()
        arrays[column][0] = bad
        with pytest.raises(ValueError, match='non-finite'):
            ops._points('cpu', arrays['x'], arrays['y'], arrays['depth'], arrays['reprojection_error'], arrays['view'], 3)


def test_views_out_of_range_are_refused_before_the_upload():
    g, configs, raw = ref.load_case('ndc_sparse')
    p = dp.collect_points(raw)
    for bad in (-1, 3):
        view = p['view'].copy()
        view[7] = bad
        with pytest.raises(RuntimeError, match='outside'):
            ops._points('cpu', p['x'], p['y'], p['depth'], p['reprojection_error'], view, 3)


def test_points_of_dataframe_like_tables_are_read_in_input_order():
    class Column:                      # what the loader's pandas columns offer
        def __init__(self, a): self.a = a
        def to_numpy(self): return self.a
    g, configs, raw = ref.load_case('ndc_both')
    wrapped = copy.deepcopy(raw)
    wrapped['sparse_depth_data'] = {f: {c: Column(a) for c, a in t.items()} for f, t in raw['sparse_depth_data'].items()}
    a, b = dp.collect_points(raw), dp.collect_points(wrapped)
    assert all(numpy.array_equal(a[k], b[k]) for k in a) and a['view'].dtype == numpy.int32 and a['x'].dtype == numpy.float64
    assert list(numpy.unique(a['view'])) == [0, 1, 2] and (numpy.diff(a['view']) >= 0).all()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(REPO, 'include', 'simplenerf_train.h')).read()
    declared = set(re.findall(r'\b(snerf_[a-z_0-9]+)\s*\(', header))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.snerf_abi_version() == _lib.ABI_VERSION == 10
    for name in ('scene_images', 'rasterise_sparse_depth', 'depth_table_to_ndc'):
        assert callable(getattr(ops, name))
    assert lib.snerf_rasterise_sparse_depth_workspace_bytes(3, 48, 64) == 3 * 48 * 64 * 4
    assert lib.snerf_rasterise_sparse_depth_workspace_bytes(0, 48, 64) == 0


def test_bad_arguments_are_refused_without_a_device():
    """Every check of the entry points comes before the first launch, so it can be exercised with no GPU: null pointers, more than
    2^31-1 points, bad sizes."""
    import ctypes
    lib = _lib.load()
    one = ctypes.c_void_p(8)           # never dereferenced: the calls below fail before anything is enqueued
    null = ctypes.c_void_p(0)
    message = lambda: lib.snerf_last_error().decode()
    assert lib.snerf_scene_images(null, 4, 3, 0, one, null) < 0 and 'NULL' in message()
    assert lib.snerf_scene_images(one, 4, 5, 0, one, null) < 0 and 'channels' in message()
    args = lambda **kw: [kw.get('x', one), one, one, one, kw.get('view', one), kw.get('points', 5), 1.0, kw.get('divisor', 1.0),
                         kw.get('table', one), 1.0, kw.get('views', 3), 4, 4, kw.get('depths', one), one, kw.get('ndc', null),
                         kw.get('workspace', one), null]
    for kw, word in (({'x': null}, 'NULL'), ({'view': null}, 'NULL'), ({'depths': null}, 'NULL'), ({'workspace': null}, 'NULL'),
                     ({'points': 2 ** 31}, '2^31-1'), ({'points': -1}, '2^31-1'), ({'views': 0}, 'sizes'), ({'divisor': 0.0}, 'divisor'),
                     ({'ndc': one, 'table': null}, 'camera table')):
        assert lib.snerf_rasterise_sparse_depth(*args(**kw)) < 0 and word in message(), (kw, message())
    assert lib.snerf_depth_table_to_ndc(one, null, 3, 4, 4, 1.0, one, null) < 0 and 'NULL' in message()
    assert lib.snerf_depth_table_to_ndc(one, one, 3, 0, 4, 1.0, one, null) < 0 and 'sizes' in message()
