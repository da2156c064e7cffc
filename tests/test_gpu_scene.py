"""The scene stage on the device (csrc/scene.hip, DataPreprocessor01): every table, image, batch and test frame against the fixtures
made by running the reference's DataPreprocessor (tools/make_golden_scene.py), bit for bit -- the arithmetic is the reference's
fp32 / fp64 operations in its order (tests/test_scene_host.py holds the numpy restatement to the same fixtures on the CPU)."""
import json

import numpy
import pytest
import torch

from simplenerf_amd import harness, ops, optim, synth
from simplenerf_amd.data_preprocessors.BatchAssembler01 import BatchAssembler
from simplenerf_amd.data_preprocessors.DataPreprocessor01 import DataPreprocessor, collect_points
from tests import scene_reference as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def assert_same_bits(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else numpy.asarray(got)
    want = numpy.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == numpy.float32:
        differing = int((ref.bits(got) != ref.bits(want)).sum())
        assert differing == 0, f'{what}: {differing} of {got.size} entries differ in their bits'
    else:
        assert numpy.array_equal(got, want), what


@pytest.fixture(scope='module', params=ref.CASES)
def case(request):
    g, configs, raw = ref.load_case(request.param)
    return request.param, g, configs, raw


def camera_table(g):
    h, w = (int(x) for x in g['raw_resolution'])
    return ops.camera_table(torch.from_numpy(g['intrinsics']).to(DEV), torch.from_numpy(g['poses']).to(DEV), (h, w)), h, w


def rasterised(g, raw, points=None):
    table, h, w = camera_table(g)
    p = collect_points(raw) if points is None else points
    return ops.rasterise_sparse_depth(p['x'], p['y'], p['depth'], p['reprojection_error'], p['view'], 3, (h, w), scale=float(g['sc']),
                                      table=table, near=1.0)


# ------------------------------------------------------------------------------------------------ each kernel on the fixture's inputs
def test_images_equal_the_reference(case):
    name, g, configs, raw = case
    images = torch.from_numpy(raw['nerf_data']['images']).to(DEV)
    assert_same_bits(ops.scene_images(images, configs['model']['white_bkgd']), g['images'], f'{name} images')
    if images.shape[-1] == 4:      # RGBA without the white background: the first three channels
        assert_same_bits(ops.scene_images(images, False), ref.prepare_images(raw['nerf_data']['images'], False), 'rgba, no background')


@pytest.mark.parametrize('name', ref.SPARSE_CASES)
def test_sparse_tables_equal_the_reference(name):
    g, configs, raw = ref.load_case(name)
    out = rasterised(g, raw)
    assert_same_bits(out['depths'], g['sparse_depths'], 'sparse depths')
    assert_same_bits(out['errors'], g['sparse_errors'], 'sparse errors')
    assert_same_bits(out['depths_ndc'], g['sparse_depths_ndc'], 'sparse depths, NDC')
    again = rasterised(g, raw)                                     # a second run: identical bits
    for key in out:
        assert torch.equal(out[key].view(torch.int32), again[key].view(torch.int32)), key
    # without a camera table there is no NDC table and the other two do not change
    h, w = raw['nerf_data']['resolution']
    p = collect_points(raw)
    plain = ops.rasterise_sparse_depth(p['x'], p['y'], p['depth'], p['reprojection_error'], p['view'], 3, (h, w), scale=float(g['sc']),
                                       device=DEV)
    assert sorted(plain) == ['depths', 'errors'] and torch.equal(plain['depths'], out['depths']) and torch.equal(plain['errors'], out['errors'])


def test_duplicates_half_way_points_clipped_points_and_the_missing_frame():
    """scene_prep_ndc_sparse's planted points, one by one, on the device's table (tests/test_scene_host.py: the same on the fixture)."""
    g, configs, raw = ref.load_case('ndc_sparse')
    h, w = raw['nerf_data']['resolution']
    out = rasterised(g, raw)
    table, errors = out['depths'].cpu().numpy().reshape(3, h, w), out['errors'].cpu().numpy().reshape(3, h, w)
    value = lambda d: numpy.float32(d * float(g['sc']))
    assert table[0, 5, 10] == value(4.5) and errors[0, 5, 10] == numpy.float32(0.7)      # duplicate pixel: an exact repeat, the later one
    assert table[0, 7, 20] == value(3.3)                                                 # duplicate pixel: three points, the last
    assert table[0, 12, 2] == value(3.4) and table[0, 13, 4] == value(3.5) and table[0, 12, 3] == -1      # half-way points: to even
    assert table[0, 0, 30] == value(3.6) and table[0, 0, 31] == value(3.7)
    assert table[0, 20, 0] == value(3.8) and table[0, 21, w - 1] == value(3.9)           # clipped points: left, right,
    assert table[0, 0, 40] == value(4.0) and table[0, h - 1, 41] == value(4.1)           # above, below
    assert (table[1] == -1).all() and (errors[1] == -1).all()                            # the missing frame
    assert (out['depths_ndc'].cpu().numpy().reshape(3, h, w)[1] == -1).all()


@pytest.mark.parametrize('name', ref.SPARSE_CASES)
def test_last_point_wins_in_both_directions(name):
    """The points of each view reversed: the restatement's result for the reversed order, so the winner is the later point, not the
    larger or smaller value."""
    g, configs, raw = ref.load_case(name)
    h, w = raw['nerf_data']['resolution']
    p = collect_points(raw)
    order = numpy.concatenate([numpy.flatnonzero(p['view'] == v)[::-1] for v in range(3)])
    reversed_points = {k: numpy.ascontiguousarray(a[order]) for k, a in p.items()}
    out = rasterised(g, raw, reversed_points)
    depths, errors = ref.rasterise(*(reversed_points[k] for k in ref.COLUMNS), reversed_points['view'], 3, h, w, scale=float(g['sc']))
    assert_same_bits(out['depths'], depths, 'reversed depths')
    assert_same_bits(out['errors'], errors, 'reversed errors')
    forward = ref.rasterise(*(p[k] for k in ref.COLUMNS), p['view'], 3, h, w, scale=float(g['sc']))[0]
    if name == 'ndc_sparse':        # the scene with planted shared pixels: there the order matters
        assert (ref.bits(forward) != ref.bits(depths)).any()


def test_many_points_on_few_pixels_over_many_blocks():
    """20 000 points on 3 x 24 x 32 pixels (every pixel contested, 79 blocks of points) with a downsampling divisor: the restatement."""
    g, configs, raw = ref.load_case('ndc_both')
    h, w = raw['nerf_data']['resolution']
    rng = numpy.random.RandomState(5)
    count = 20000
    p = {'x': rng.uniform(-4, 2 * w + 4, count), 'y': rng.uniform(-4, 2 * h + 4, count), 'depth': rng.uniform(1, 9, count),
         'reprojection_error': rng.uniform(0, 3, count), 'view': rng.randint(0, 3, count).astype(numpy.int32)}
    p['x'][:64] = numpy.arange(64) + 0.5             # exact halves before the division, and after it
    p['y'][64:128] = 2 * numpy.arange(64) + 1.0
    table, _, _ = camera_table(g)
    out = ops.rasterise_sparse_depth(p['x'], p['y'], p['depth'], p['reprojection_error'], p['view'], 3, (h, w), scale=0.37, divisor=2.0,
                                     table=table, near=1.0)
    depths, errors = ref.rasterise(*(p[k] for k in ref.COLUMNS), p['view'], 3, h, w, scale=0.37, divisor=2.0)
    assert_same_bits(out['depths'], depths, 'contested depths')
    assert_same_bits(out['errors'], errors, 'contested errors')
    oz, dz = ref.pixel_rays_z(g['intrinsics'], g['poses'], h, w)
    assert_same_bits(out['depths_ndc'], ref.depth_to_ndc(depths, oz, dz, 1), 'contested depths, NDC')
    assert (depths > 0).mean() > 0.99
    on_device = {k: torch.from_numpy(a).to(DEV) for k, a in p.items()}          # the same from device tensors
    again = ops.rasterise_sparse_depth(on_device['x'], on_device['y'], on_device['depth'], on_device['reprojection_error'],
                                       on_device['view'], 3, (h, w), scale=0.37, divisor=2.0, table=table, near=1.0)
    assert all(torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)) for k in out)


def test_no_points_yield_tables_of_minus_one():
    g, configs, raw = ref.load_case('ndc_sparse')
    table, h, w = camera_table(g)
    none = numpy.zeros((0,))
    out = ops.rasterise_sparse_depth(none, none, none, none, numpy.zeros((0,), dtype=numpy.int32), 3, (h, w), table=table)
    for key in ('depths', 'errors', 'depths_ndc'):
        assert out[key].shape == (3 * h * w,) and bool((out[key] == -1).all()), key
    everything_missing = dict(raw, sparse_depth_data={})                                # the same through the class
    pp = DataPreprocessor(configs_for(configs), 'train', everything_missing, device=DEV)
    assert bool((pp.scene['sparse_depths'] == -1).all()) and bool((pp.scene['sparse_depths_ndc'] == -1).all())


@pytest.mark.parametrize('name', ref.DENSE_CASES)
def test_dense_depth_to_ndc_equals_the_reference(name):
    g, configs, raw = ref.load_case(name)
    table, h, w = camera_table(g)
    depths = torch.from_numpy(g['dense_depths']).to(DEV)
    if 'dense_depths_ndc' in g:
        assert_same_bits(ops.depth_table_to_ndc(depths, table, (h, w), float(g['near'])), g['dense_depths_ndc'], 'dense depths, NDC')
        shaped = ops.depth_table_to_ndc(depths.reshape(3, h, w), table, (h, w), float(g['near']))
        assert shaped.shape == (3, h, w)
    else:        # a world-space scene has no NDC table in the reference: the restatement, with the scene's near
        oz, dz = ref.pixel_rays_z(g['intrinsics'], g['poses'], h, w)
        assert_same_bits(ops.depth_table_to_ndc(depths, table, (h, w), float(g['near'])),
                         ref.depth_to_ndc(g['dense_depths'], oz, dz, float(g['near'])), 'dense depths, NDC (restated)')
    empty = torch.full((3 * h * w,), -1.0, device=DEV)                                  # all -1 stays all -1
    assert bool((ops.depth_table_to_ndc(empty, table, (h, w), float(g['near'])) == -1).all())


# ------------------------------------------------------------------------------------------------ end to end
def configs_for(configs, **extra):
    out = json.loads(json.dumps(configs))
    out.update(extra)
    return out


def test_batches_from_raw_data_equal_the_references(case):
    """DataPreprocessor(configs, 'train', raw) with the index lists the reference drew returns its three batches bit for bit."""
    name, g, configs, raw = case
    pp = DataPreprocessor(configs, 'train', raw, device=DEV)
    for key in ('poses', 'intrinsics', 'images'):
        assert_same_bits(pp.scene[key], g[key], f'{name} scene {key}')
    for key in ('sparse_depths', 'sparse_errors', 'sparse_depths_ndc', 'dense_depths', 'dense_depth_weights', 'dense_depths_ndc'):
        assert (key in g) == (pp.scene.get(key) is not None), key
        if key in g:
            assert_same_bits(pp.scene[key], g[key], f'{name} scene {key}')
    sparse = 'sparse_depth' in configs['data_loader']
    for b in range(3):
        indices, pixel_rows = g[f'batch{b}_indices'], g[f'batch{b}_indices_mask_nerf']
        replay = {'indices': torch.from_numpy(indices[pixel_rows])}
        if sparse:
            replay['indices_sparse'] = torch.from_numpy(indices[g[f'batch{b}_indices_mask_sparse_depth']])
        batch = pp.get_next_batch(b, **replay)
        expected = {k[len(f'batch{b}_'):]: v for k, v in g.items() if k.startswith(f'batch{b}_')}
        assert len(expected) >= 11
        for key, want in expected.items():
            got = batch[key]
            if not isinstance(got, torch.Tensor):
                assert got == want, key
            else:
                assert_same_bits(got, want, f'{name} batch {b} {key}')
        common = batch['common_data']
        assert_same_bits(common['poses'][0], g['poses'], 'common poses')
        assert_same_bits(common['images'][0], g['images'], 'common images')
    mine, theirs = pp.get_model_configs(), json.loads(str(g['model_configs_json']))
    assert list(mine) == list(theirs) and mine['intrinsic'] == theirs['intrinsic'] and mine['near'] == theirs['near']


def test_create_test_data_equals_the_references(case):
    name, g, configs, raw = case
    trained = DataPreprocessor(configs, 'train', raw, device=DEV)
    saved = json.loads(json.dumps(trained.get_model_configs()))
    for pp in (trained, DataPreprocessor(configs, 'test', model_configs=saved, device=DEV)):
        batch = pp.create_test_data(g['test_pose'])
        expected = {k[len('test_'):]: v for k, v in g.items() if k.startswith('test_') and k != 'test_pose'}
        assert sorted(batch) == sorted(expected) and len(expected) == (9 if configs['data_loader']['ndc'] else 5)
        for key, want in expected.items():
            assert_same_bits(batch[key], want, f'{name} test frame {key}')
    processed = g['poses'][1]                       # an already processed pose passes through
    rays = trained.create_test_data(processed, preprocess_pose=False, intrinsic=g['intrinsics'][1])
    pixels = torch.arange(rays['rays_o'].shape[0]) + rays['rays_o'].shape[0]
    assert torch.equal(rays['rays_d'], trained.get_next_batch(0, indices=pixels)['rays_d'])


def test_training_from_raw_data_equals_training_from_the_references_tables():
    """Five iterations of harness.train_one_iter fed by the DataPreprocessor give, bit for bit, the losses of five fed by a
    BatchAssembler over the fixture's tables."""
    from simplenerf_amd.loss_functions.LossComputer01 import LossComputer
    from simplenerf_amd.models.ModelFactory import get_model
    g, configs, raw = ref.load_case('ndc_sparse')
    cfg = synth.training_configs('fp32', num_rays=96, num_sparse=32)
    cfg['data_loader'].update(configs['data_loader'])
    cfg['model']['white_bkgd'] = configs['model']['white_bkgd']
    cfg['sub_batch_size'] = 128
    h, w = raw['nerf_data']['resolution']
    scene = {'resolution': (h, w), 'frame_nums': [int(f) for f in raw['frame_nums']]}
    scene.update({k: g[k] for k in ('poses', 'intrinsics', 'images', 'sparse_depths', 'sparse_errors', 'sparse_depths_ndc')})
    scene.update({k: float(g[k]) for k in ('near', 'far', 'near_ndc', 'far_ndc')})
    feeds = [DataPreprocessor(cfg, 'train', raw, device=DEV), BatchAssembler(cfg, scene, DEV)]
    runs = []
    for feed in feeds:
        model = get_model(cfg, None)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 9, 200.0, 8.0).items()})
        model = model.to(DEV).train()
        losses, opt = LossComputer(cfg), optim.Adam(list(model.parameters()), lr=1e-3)
        totals = [harness.train_one_iter(model, losses, opt, feed.get_next_batch(it), 128) for it in range(20000, 20005)]
        runs.append([{k: float(v) for k, v in t.items()} for t in totals])
    assert runs[0] == runs[1]
    assert len({t['TotalLoss'] for t in runs[0]}) == 5 and all(numpy.isfinite(t['TotalLoss']) for t in runs[0])
