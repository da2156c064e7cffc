"""The validation mode, the 8-bit conversion and the trainer's two frame loops on a real MI355X, against the fixtures made by running
the reference (tools/make_golden_validation.py): validation-mode scenes and per-image batches bit for bit, ``ops.maps_to_u8`` against
the reference's previews and against the numpy expressions evaluated here, ``harness.run_validation`` / ``save_sample_images`` /
``save_depth`` on the fixture's model and scene.

Float maps of the pass are held to the gates of tests/test_gpu_model.py for this model path (fp32, the model's own resampling):
colour-like values 1e-4 and NDC depths 1e-3, world depths of the NDC scene relative to their magnitude on rays with acc > 1e-2;
coarse-level maps on every ray, fine-level maps on all but MAX_OUTLIER_RAYS of the rays (MAX_OUTLIER_RAYS_WORLD for the fine world
depth and variance) -- that module's gate for fine outputs whose resampled depths are not pinned to the reference's (its docstring
and DESIGN section 4: sample_pdf's ``denom < 1e-5`` branch is decided by the last bit of a running fp32 sum).  Measured on this
fixture's five 768-ray frames: depth_ndc_fine over 1e-3 on 1 + 4 rays and rgb_fine over 1e-4 on 2, six of the seven on rays whose
fine depths differ from the oracle's by more than 1e-5 -- and the oracle, the reference's arithmetic restated on the CPU, is itself
over the bound against the fixture on 2 rays of frame 8; every coarse-level map holds on every ray.  The loss maps are
functions of those outputs and inherit their bounds: an MSE01 map is mean_c (rgb - target)^2, so it moves by at most
2 max|rgb - target| RGB_TOL + RGB_TOL^2 (the fine one on all but MAX_OUTLIER_RAYS of the rays); a CoarseFineConsistencyLoss01 map is
(depth_coarse - depth_fine)^2, so it moves by at most 2 |depth_coarse - depth_fine| t + t^2 with t the sum of the two depths' own
bounds, on the rays where both depths are gated, and like the fine world depth it is allowed MAX_OUTLIER_RAYS_WORLD of outliers."""
import os

import numpy
import pytest
import torch

from simplenerf_amd import harness, ops, synth
from simplenerf_amd.data_preprocessors.DataPreprocessor01 import DataPreprocessor
from simplenerf_amd.loss_functions.LossComputer01 import LossComputer
from simplenerf_amd.models.ModelFactory import get_model
from tests import util
from tests import validation_reference as ref
from tests.test_gpu_losses import REL
from tests.test_gpu_model import DEPTH_TOL, MAX_OUTLIER_RAYS, MAX_OUTLIER_RAYS_WORLD, RGB_TOL, per_ray_violation
from tests.test_gpu_scene import assert_same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ITER_NUM = 41


@pytest.fixture(scope='module', params=ref.CASES)
def case(request):
    return (request.param,) + ref.load_prep(request.param)


# ------------------------------------------------------------------------------------------------ the validation-mode preprocessor
def assert_batch(batch, g, prefix, what):
    expected = {k[len(prefix) + 1:]: v for k, v in g.items() if k.startswith(prefix + '_') and not k.endswith('_keys')}
    names = set(g[f'{prefix}_keys'].tolist())
    assert set(expected) | {'common_data'} == names and len(expected) >= 11
    assert set(batch) - ref.BATCH_KEYS_OF_THIS_BUILD == names, (what, sorted(set(batch) ^ names))          # absent keys are absent
    for key, want in expected.items():
        got = batch[key]
        if not isinstance(got, torch.Tensor):
            assert got == want, (what, key)
        else:
            assert_same_bits(got, want, f'{what} {key}')


def test_validation_scene_and_batches_equal_the_reference(case):
    name, g, configs, train_raw, held_raw = case
    saved = ref.model_configs(g)
    pp = DataPreprocessor(configs, 'validation', held_raw, saved, device=DEV)
    assert pp.mode == 'validation' and pp.get_model_configs() is saved
    for key in ('images', 'poses', 'intrinsics'):
        assert_same_bits(pp.scene[key], g[f'val_{key}'], f'{name} validation scene {key}')
    assert all(pp.scene.get(k) is None for k in ('sparse_depths', 'sparse_errors', 'sparse_depths_ndc', 'dense_depths', 'dense_depth_weights'))
    assert (pp.scene['near'], pp.scene['far']) == (float(g['val_near']), float(g['val_far']))
    view = pp.preprocessed_data_dict
    assert view['frame_nums'].tolist() == held_raw['frame_nums'].tolist() and numpy.array_equal(view['nerf_data']['poses'], g['val_poses'])
    for frame in held_raw['frame_nums'].tolist():
        batch = pp.get_next_batch(0, frame)
        assert_batch(batch, g, f'val{frame}', f'{name} held-out frame {frame}')
        assert batch['common_data'] == {} and g[f'val{frame}_common_data_keys'].size == 0
        assert not any(k.startswith(('sparse_', 'dense_')) or k == 'indices_mask_sparse_depth' for k in batch)
    # the training views through the train-mode preprocessor, as :302 validates them: the shared scene is there
    trained = DataPreprocessor(configs, 'train', train_raw, device=DEV)
    frame = int(train_raw['frame_nums'][1])
    batch = trained.get_next_batch(0, frame)
    assert_batch(batch, g, f'train{frame}', f'{name} training frame {frame}')
    assert set(g[f'train{frame}_common_data_keys'].tolist()) == set(batch['common_data']) >= {'images', 'intrinsics', 'poses'}
    assert trained.mode == 'train' and set(trained.preprocessed_data_dict['nerf_data']) >= {'poses', 'resolution', 'sc'}
    # start_training's order (src/Trainer01.py:503-511): the validation preprocessor from OUR train-mode model configs
    again = DataPreprocessor(configs, 'validation', held_raw, trained.get_model_configs(), device=DEV)
    frame = int(held_raw['frame_nums'][1])
    assert_batch(again.get_next_batch(0, frame), g, f'val{frame}', f'{name} held-out frame {frame}, own model configs')
    # without an image number: pixel rows of its own views only, from its own index stream
    h, w = held_raw['nerf_data']['resolution']
    drawn = again.get_next_batch(0)
    assert drawn['common_data'] == {} and 'indices_mask_sparse_depth' not in drawn and bool(drawn['indices_mask_nerf'].all())
    assert drawn['indices'].shape[0] == configs['data_loader']['num_rays'] and int(drawn['indices'].max()) < 2 * h * w
    assert int(drawn['pixel_id'][:, 0].max()) <= 1


# ------------------------------------------------------------------------------------------------ ops.maps_to_u8
def expected_u8(maps, modes):
    return numpy.stack([ref.colour_u8(m) if mode == 0 else ref.preview_u8(m) for m, mode in zip(maps, modes)])


def converted(maps, modes):
    out, status = ops.maps_to_u8(torch.from_numpy(numpy.ascontiguousarray(maps)).to(DEV), modes)
    assert out.dtype == torch.uint8 and status.dtype == torch.int32 and out.shape == maps.shape and status.shape == (maps.shape[0],)
    return out.cpu().numpy(), status.cpu().numpy()


def test_maps_to_u8_gives_the_references_previews_of_its_float_maps():
    g = util.load('validation_pass.npz')
    for tag in ('val', 'train'):
        files = ref.written(g, tag)
        names = sorted(name for name in files if name.endswith('.npy'))
        colours = sorted(k for k in g if k.startswith(f'{tag}_rgb/'))
        assert len(names) == (22 if tag == 'val' else 33) and len(colours) == (4 if tag == 'val' else 6)
        rows = [files[name].reshape(-1) for name in names] + [row for k in colours for row in g[k].reshape(3, -1)]
        modes = [1] * len(names) + [0] * (3 * len(colours))
        out, status = converted(numpy.stack(rows), modes)              # all maps of the pass in one call
        assert not status.any()
        for i, name in enumerate(names):
            assert numpy.array_equal(out[i].reshape(24, 32), files[name[:-4] + '.png']), name
        for j, k in enumerate(colours):
            got = out[len(names) + 3 * j:len(names) + 3 * j + 3].reshape(24, 32, 3)
            assert numpy.array_equal(got, files[k[len(tag) + 5:]]), k


@pytest.mark.parametrize('count', [1, 9])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 4097])
def test_maps_to_u8_equals_numpy_on_every_length(n, count):
    rng = numpy.random.RandomState(n + count)
    modes = [(k + 1) % 2 for k in range(count)]                        # mode 1 first
    maps = numpy.stack([rng.uniform(0, 1, n) if mode == 0 else rng.uniform(0, 37.5, n) for mode in modes]).astype(numpy.float32)
    out, status = converted(maps, modes)
    assert numpy.array_equal(out, expected_u8(maps, modes)) and not status.any()
    assert all(out[k].max() == 255 for k in range(count) if modes[k] == 1)


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_maps_to_u8_on_maps_that_do_not_start_on_a_16_byte_boundary(offset):
    rng = numpy.random.RandomState(offset)
    count, n = 3, 1021                                                 # odd length: every map starts at another offset from a boundary
    modes = [1, 0, 1]
    storage = torch.from_numpy(rng.uniform(0, 1, offset + count * n).astype(numpy.float32)).to(DEV)
    view = storage[offset:].reshape(count, n)
    assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
    out, status = ops.maps_to_u8(view, modes)
    assert numpy.array_equal(out.cpu().numpy(), expected_u8(view.cpu().numpy(), modes)) and not bool(status.any())


def test_maps_to_u8_rounds_exact_halves_to_even():
    k = numpy.arange(4096) % 255
    colour = ((k + 0.5).astype(numpy.float32) / numpy.float32(255))
    scaled = (k + 0.5).astype(numpy.float32)
    scaled[-1] = 255.0                                                 # the maximum: x / 255 * 255
    maps = numpy.stack([colour, scaled])
    ties = [int(((colour * numpy.float32(255)) % 1 == 0.5).sum()), int(((scaled / scaled.max() * numpy.float32(255)) % 1 == 0.5).sum())]
    assert min(ties) > 500, ties                                       # the float32 products really land on .5
    out, status = converted(maps, [0, 1])
    want = expected_u8(maps, [0, 1])
    assert numpy.array_equal(out, want) and not status.any()
    on_tie = (colour * numpy.float32(255)) % 1 == 0.5
    assert (want[0][on_tie] % 2 == 0).all() and {int(v) for v in want[0][on_tie]} >= {0, 2, 100, 254}


def test_maps_to_u8_single_non_zero_element():
    for n, at in ((4097, 0), (4097, 4096), (65, 33), (1, 0)):
        maps = numpy.zeros((2, n), dtype=numpy.float32)
        maps[0, at] = 3.7
        maps[1, at] = 1e-30
        out, status = converted(maps, [1, 1])
        assert numpy.array_equal(out, expected_u8(maps, [1, 1])) and not status.any()
        assert out[0, at] == 255 and out[0].astype(numpy.int64).sum() == 255 and out[1, at] == 255


def test_maps_to_u8_saturates_out_of_range_colours():
    values = numpy.array([-0.5, -1e-3, 1.5, 300.0, 1.0019, -numpy.inf, numpy.inf, numpy.nan, 0.25, 1.0, -0.0], dtype=numpy.float32)
    want = numpy.array([0, 0, 255, 255, 255, 0, 255, 0, 64, 255, 0], dtype=numpy.uint8)
    maps = numpy.stack([values, numpy.full_like(values, 0.5)])
    out, status = converted(maps, [0, 0])
    assert numpy.array_equal(out[0], want) and (out[1] == 128).all() and not status.any()
    # negatives of a mode-1 map with a positive maximum saturate to 0 as well
    out, status = converted(numpy.array([[-3.0, 2.0, 1.0, -numpy.inf]], dtype=numpy.float32), [1])
    assert out.tolist() == [[0, 255, 128, 0]] and status.tolist() == [0]


def test_maps_to_u8_degenerate_maps_give_zeros_and_a_status_and_leave_their_neighbours_alone():
    n = 777
    rng = numpy.random.RandomState(9)
    good = lambda: rng.uniform(0, 4, n).astype(numpy.float32)
    with_nan, with_inf = good(), good()
    with_nan[700], with_inf[3] = numpy.nan, numpy.inf
    maps = numpy.stack([good(), numpy.zeros(n, dtype=numpy.float32), good(), -good(), good(), with_nan, with_inf, good(),
                        numpy.full(n, numpy.nan, dtype=numpy.float32)])
    modes = [1, 1, 0, 1, 1, 1, 1, 1, 1]
    maps[2] /= 4
    out, status = converted(maps, modes)
    assert status.tolist() == [0, 1, 0, 1, 0, 1, 1, 0, 1]
    for k, bad in enumerate(status.tolist()):
        if bad:
            assert not out[k].any(), k
        else:
            assert numpy.array_equal(out[k], expected_u8(maps[k:k + 1], modes[k:k + 1])[0]), k
    # a degenerate colour map (mode 0) has no status: it saturates value by value
    out, status = converted(numpy.stack([numpy.zeros(n, dtype=numpy.float32), -good()]), [0, 0])
    assert not out.any() and status.tolist() == [0, 0]


def test_maps_to_u8_empty_calls_and_bad_arguments():
    out, status = ops.maps_to_u8(torch.empty((0, 5), device=DEV), [])
    assert out.shape == (0, 5) and status.shape == (0,)
    out, status = ops.maps_to_u8(torch.empty((3, 0), device=DEV), [0, 1, 1])
    assert out.shape == (3, 0) and status.tolist() == [0, 0, 0]
    with pytest.raises(RuntimeError, match='modes'):
        ops.maps_to_u8(torch.zeros((2, 4), device=DEV), [1])
    with pytest.raises(RuntimeError, match='modes'):
        ops.maps_to_u8(torch.zeros((2, 4), device=DEV), [1, 2])
    with pytest.raises(RuntimeError, match='GPU'):
        ops.maps_to_u8(torch.zeros((2, 4)), [1, 1])
    with pytest.raises(RuntimeError, match='float32'):
        ops.maps_to_u8(torch.zeros((2, 4), device=DEV, dtype=torch.float64), [1, 1])


def test_save_depth_writes_the_same_bytes_from_the_device_as_from_the_host(tmp_path):
    depth = numpy.random.RandomState(2).uniform(0, 9, (37, 53)).astype(numpy.float32)
    on_device = torch.from_numpy(depth).to(DEV)
    for kind, argument in (('host', depth), ('device', on_device)):
        harness.save_depth(tmp_path / kind / 'a.png', argument)
        harness.save_depth(tmp_path / kind / 'b.npy', argument, as_png=True)
        harness.save_depth(tmp_path / kind / 'c.npy', argument)
    for name in ('a.png', 'b.npy', 'b.png', 'c.npy'):
        assert (tmp_path / 'host' / name).read_bytes() == (tmp_path / 'device' / name).read_bytes(), name
    assert not (tmp_path / 'device' / 'c.png').exists()
    assert numpy.array_equal(ref.decode_png((tmp_path / 'device' / 'b.png').read_bytes()), ref.preview_u8(depth))
    assert numpy.array_equal(numpy.load(tmp_path / 'device' / 'b.npy'), depth)


# ------------------------------------------------------------------------------------------------ the validation pass
@pytest.fixture(scope='module')
def validated(tmp_path_factory):
    """harness.run_validation over the validation and the train preprocessor of the NDC fixture scene, once for the module."""
    g, configs, train_raw, held_raw = ref.load_prep('ndc')
    gp = util.load('validation_pass.npz')
    configs = synth.with_overrides(configs, hip_precision='fp32')
    model = get_model(configs, None)
    result = model.load_state_dict(ref.pass_weights(configs, gp), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    model = model.to(DEV).train()
    trained = DataPreprocessor(configs, 'train', train_raw, device=DEV)
    held = DataPreprocessor(configs, 'validation', held_raw, trained.get_model_configs(), device=DEV)
    losses = LossComputer(configs)
    runs = {}
    for tag, loader in (('val', held), ('train', trained)):
        keep, directory = {}, tmp_path_factory.mktemp(tag)
        totals = harness.run_validation(model, losses, loader, ITER_NUM, configs, save_dirpath=directory, keep=keep)
        runs[tag] = {'totals': totals, 'keep': keep, 'directory': directory, 'training_after': model.training,
                     'frames': loader.preprocessed_data_dict['frame_nums'].tolist()}
    return {'g': gp, 'configs': configs, 'model': model, 'trained': trained, 'held': held, 'runs': runs,
            'targets': {'val': held.scene['images'].cpu().numpy(), 'train': trained.scene['images'].cpu().numpy()}}


def output_key(stem: str) -> str:
    directory, name = stem.split('/')
    level = 'coarse' if '_coarse_' in name else 'fine'
    kind = {'predicted_frames': 'rgb', 'predicted_depths': 'depth', 'predicted_depths_variance': 'depth_var'}[directory]
    return f'{kind}{"_ndc" if "_ndc_" in name else ""}_{level}'


def depth_bound(key, want):
    """The bound per_ray_violation holds ``key`` to, per ray (NDC scene): absolute for the NDC forms, relative to the magnitude for
    the world forms (10x looser for the world variance)."""
    if key.startswith(('depth_ndc', 'depth_var_ndc')):
        return numpy.full(want.shape, DEPTH_TOL)
    return (10 if key.startswith('depth_var') else 1) * DEPTH_TOL * numpy.maximum(numpy.abs(want.astype(numpy.float64)), 1.0)


@pytest.mark.parametrize('tag', ['val', 'train'])
def test_run_validation_keeps_the_references_maps(validated, tag):
    g, run = validated['g'], validated['runs'][tag]
    files = ref.written(g, tag)
    keep = run['keep']
    assert run['training_after'] and validated['model'].training
    assert {stem for _, stem in keep} == {os.path.splitext(name)[0] for name in files}          # the reference's file stems
    assert {frame for frame, _ in keep} == set(run['frames']) and len(keep) == len(run['frames']) * 13
    worst = (0.0, 'none over tolerance')
    for (frame, stem), arrays in sorted(keep.items()):
        assert f'{frame:04}_' in stem
        colour = stem.startswith('predicted_frames/')
        got, u8 = arrays['float'], arrays['u8']
        assert got.dtype == numpy.float32 and u8.dtype == numpy.uint8 and got.shape == u8.shape == ((24, 32, 3) if colour else (24, 32))
        # every 8-bit array is the numpy expression of the float map it came from
        assert numpy.array_equal(u8, ref.colour_u8(got) if colour else ref.preview_u8(got)), stem
        want = g[f'{tag}_rgb/{stem}.png'] if colour else files[stem + '.npy']
        acc = {level: g[f'{tag}_acc_{level}_{frame}'].astype(numpy.float64) for level in ('coarse', 'fine')}
        if stem.startswith('Losses/'):
            continue                                                   # gated below, from the outputs' own bounds
        key = output_key(stem)
        level = key.rsplit('_', 1)[1]
        bad = per_ray_violation(key, torch.from_numpy(got.reshape(768, -1)), want.reshape(768, -1), acc[level], ndc=True)
        if level == 'coarse':
            assert not bad.any(), (stem, int(bad.sum()), util.linf(got, want))                 # every ray
        else:
            bound = MAX_OUTLIER_RAYS_WORLD if key in ('depth_fine', 'depth_var_fine') else MAX_OUTLIER_RAYS
            worst = max(worst, (float(bad.mean()) / bound, f'{key} frame {frame}: {int(bad.sum())}/768 rays over tolerance [{bound}]'))
            assert bad.mean() <= bound, (stem, float(bad.mean()))
    util.observe(f'validation pass {tag}, worst fine map', worst[1])
    observed = {stem.split('/')[0] for _, stem in keep}
    assert observed == {'predicted_frames', 'predicted_depths', 'predicted_depths_variance', 'Losses'}


@pytest.mark.parametrize('tag', ['val', 'train'])
def test_run_validation_loss_maps_follow_from_the_outputs(validated, tag):
    g, run = validated['g'], validated['runs'][tag]
    files, keep = ref.written(g, tag), run['keep']
    label = f'Iter{ITER_NUM + 1:05}'
    for index, frame in enumerate(run['frames']):
        target = validated['targets'][tag][index].reshape(768, 3).astype(numpy.float64)
        acc = {level: g[f'{tag}_acc_{level}_{frame}'].astype(numpy.float64) for level in ('coarse', 'fine')}
        for level in ('coarse', 'fine'):
            stem = f'Losses/MSE01_{level}_{frame:04}_{label}'
            rgb = g[f'{tag}_rgb/predicted_frames/{frame:04}_{level}_{label}.png'].reshape(768, 3).astype(numpy.float64)
            bound = 2 * numpy.abs(rgb - target).max(1) * RGB_TOL + RGB_TOL ** 2
            error = numpy.abs(keep[(frame, stem)]['float'].reshape(768).astype(numpy.float64) - files[stem + '.npy'].reshape(768))
            bad = error > bound + 1e-7                                 # (+ the fp32 rounding of the map itself)
            assert bad.mean() <= (0 if level == 'coarse' else MAX_OUTLIER_RAYS), (stem, int(bad.sum()), float((error - bound).max()))
        stem = f'Losses/CoarseFineConsistencyLoss01_{frame:04}_{label}'
        depths = {level: files[f'predicted_depths/{frame:04}_{level}_{label}.npy'].reshape(768).astype(numpy.float64) for level in ('coarse', 'fine')}
        t = depth_bound('depth_coarse', depths['coarse']) + depth_bound('depth_fine', depths['fine'])
        bound = 2 * numpy.abs(depths['coarse'] - depths['fine']) * t + t ** 2
        want = files[stem + '.npy'].reshape(768).astype(numpy.float64)
        error = numpy.abs(keep[(frame, stem)]['float'].reshape(768).astype(numpy.float64) - want)
        gated = (acc['coarse'] > 1e-2) & (acc['fine'] > 1e-2)
        bad = gated & (error > bound + 1e-6 * numpy.abs(want))
        assert gated.mean() > 0.5 and bad.mean() <= MAX_OUTLIER_RAYS_WORLD, (stem, float(bad.mean()))


@pytest.mark.parametrize('tag', ['val', 'train'])
def test_run_validation_totals_follow_the_chunk_rule(validated, tag):
    """The returned totals against a float64 recomputation from the kept loss maps: per chunk of 200 rays (the last one 168) the mean
    of the map, the PLAIN mean of the four chunk values per frame, the mean over the frames."""
    g, run = validated['g'], validated['runs'][tag]
    keep, configs = run['keep'], validated['configs']
    label = f'Iter{ITER_NUM + 1:05}'
    chunk = configs['validation_chunk_size']
    weights = {entry['name']: entry['weight'] for entry in configs['losses']}
    assert chunk == 200 and weights == {'MSE01': 1, 'CoarseFineConsistencyLoss01': 0.1}

    def chunk_means(stem, frame):
        values = keep[(frame, stem)]['float'].reshape(768).astype(numpy.float64)
        return numpy.array([values[start:start + chunk].mean() for start in range(0, 768, chunk)])

    expected = {'MSE01': 0.0, 'CoarseFineConsistencyLoss01': 0.0, 'TotalLoss': 0.0}
    for frame in run['frames']:
        mse = chunk_means(f'Losses/MSE01_coarse_{frame:04}_{label}', frame) + chunk_means(f'Losses/MSE01_fine_{frame:04}_{label}', frame)
        consistency = chunk_means(f'Losses/CoarseFineConsistencyLoss01_{frame:04}_{label}', frame)
        assert mse.shape == (4,)
        expected['MSE01'] += mse.mean() / len(run['frames'])
        expected['CoarseFineConsistencyLoss01'] += consistency.mean() / len(run['frames'])
        expected['TotalLoss'] += (mse + 0.1 * consistency).mean() / len(run['frames'])
    totals = run['totals']
    assert list(totals) == list(expected) and all(isinstance(v, float) for v in totals.values())
    for name, want in expected.items():
        relative = abs(totals[name] - want) / abs(want)
        reference = float(g[f'{tag}_total_{name}'])
        util.observe(f'validation totals {tag} {name}', f'{relative:.2e} from the float64 chunk rule [{REL}]; the reference returned '
                                                        f'{reference:.6g}, here {totals[name]:.6g}')
        assert relative <= REL, (name, totals[name], want)


@pytest.mark.parametrize('tag', ['val', 'train'])
def test_run_validation_writes_the_references_files(validated, tag):
    g, run = validated['g'], validated['runs'][tag]
    files, keep, directory = ref.written(g, tag), run['keep'], run['directory']
    on_disk = {os.path.relpath(os.path.join(root, name), directory) for root, _, names in os.walk(directory) for name in names}
    assert on_disk == set(files)                                       # the reference's names, nothing else
    for name in sorted(on_disk):
        stem, suffix = os.path.splitext(name)
        frame = next(f for (f, s) in keep if s == stem)
        if suffix == '.png':
            assert numpy.array_equal(ref.decode_png((directory / name).read_bytes()), keep[(frame, stem)]['u8']), name
        else:
            loaded = numpy.load(directory / name)
            assert loaded.dtype == numpy.float32 and numpy.array_equal(loaded, keep[(frame, stem)]['float']), name


def test_run_validation_without_a_directory_or_keep_only_returns_the_totals(validated):
    model, configs = validated['model'], validated['configs']
    model.eval()
    totals = harness.run_validation(model, LossComputer(configs), validated['held'], ITER_NUM, configs)
    assert model.training                                              # put into train mode at the end, whatever it was (:262)
    assert totals == validated['runs']['val']['totals']


def test_save_sample_images_writes_one_set_per_view(validated, tmp_path):
    model, configs, trained, held = (validated[k] for k in ('model', 'configs', 'trained', 'held'))
    keep = {}
    harness.save_sample_images(model, configs, [trained, held], 7, tmp_path, keep=keep)
    assert model.training
    frames = trained.preprocessed_data_dict['frame_nums'].tolist() + held.preprocessed_data_dict['frame_nums'].tolist()
    names = {f'{directory}/{frame:04}{ndc}_Iter00007.png' for frame in frames for directory, ndc in
             (('predicted_frames', ''), ('predicted_depths', ''), ('predicted_depths', '_ndc'), ('predicted_depths_variance', ''),
              ('predicted_depths_variance', '_ndc'))}
    on_disk = {os.path.relpath(os.path.join(root, name), tmp_path) for root, _, files in os.walk(tmp_path) for name in files}
    assert on_disk == names and len(names) == 25
    saved = trained.get_model_configs()
    for loader in (trained, held):
        view = loader.preprocessed_data_dict
        for frame, pose in zip(view['frame_nums'].tolist(), view['nerf_data']['poses']):
            camera = {'resolution': (24, 32), 'intrinsic': numpy.array(saved['intrinsic'], dtype=numpy.float32), 'pose': pose,
                      'near': saved['near'], 'far': saved['far'], 'near_ndc': saved['near_ndc'], 'far_ndc': saved['far_ndc']}
            model.eval()
            frame_out = harness.predict_frame(model, configs, camera, DEV)
            model.train()
            image = ref.decode_png((tmp_path / f'predicted_frames/{frame:04}_Iter00007.png').read_bytes())
            assert numpy.array_equal(image, frame_out['image']) and numpy.array_equal(keep[(frame, f'predicted_frames/{frame:04}_Iter00007')]['u8'], image)
            for directory, ndc, key in (('predicted_depths', '', 'depth'), ('predicted_depths', '_ndc', 'depth_ndc'),
                                        ('predicted_depths_variance', '', 'depth_var'), ('predicted_depths_variance', '_ndc', 'depth_var_ndc')):
                preview = ref.decode_png((tmp_path / f'{directory}/{frame:04}{ndc}_Iter00007.png').read_bytes())
                assert numpy.array_equal(preview, ref.preview_u8(frame_out[key])), (frame, key)
