"""The static-camera view sweep on a real MI355X: batches with a view camera and secondary cameras against the reference's
create_test_data bit for bit, the ordinary route and ``ops.view_sweep`` against the reference's colours (tests/golden/view_sweep.npz,
tools/make_golden_view_sweep.py), the kernel's own edges (samples of several rays in one 32-sample block, a partial last block, one
ray, 37 views, white background), determinism, independence of the views and of the ray blocks, frames, the fallback route and files."""
import os

import numpy
import pytest
import torch

from simplenerf_amd import harness, ops, synth
from simplenerf_amd.data_preprocessors.DataPreprocessor01 import DataPreprocessor
from simplenerf_amd.models.ModelFactory import get_model
from tests import util
from tests import validation_reference
from tests import view_sweep_reference as ref
from tests.test_gpu_model import DEPTH_TOL, RGB_TOL, per_ray_violation

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def same_bits(a, b) -> bool:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else numpy.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else numpy.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(numpy.uint8) == b.view(numpy.uint8)).all())


@pytest.fixture(scope='module', params=ref.CASES)
def case(request):
    """One fixture case: its arrays, the fp32 model with the fixture's weights, the preprocessor and the cameras."""
    g, configs, saved, scene_configs = ref.load_case(request.param)
    model = get_model(synth.with_overrides(configs, hip_precision='fp32'), None)
    model.load_state_dict(util.golden_params(configs, g), strict=True)
    model = model.to(DEV).eval()
    dp = DataPreprocessor(scene_configs, 'test', model_configs=saved, device=DEV)
    camera = dp.camera(g['pose'], g['intrinsic'])
    view_cameras = [dp.camera(p, i) for p, i in zip(g['view_poses'], g['view_intrinsics'])]
    return {'tag': request.param, 'g': g, 'configs': model.configs, 'model': model, 'dp': dp, 'camera': camera, 'view_cameras': view_cameras,
            'ndc': bool(configs['data_loader']['ndc'])}


def keep_and_sweep(model, batch, view_dirs, z_vals_fine=None):
    """A keep-activations render of ``batch`` and one ``ops.view_sweep`` over ``view_dirs`` (V,n,3) -> (kept, out)."""
    mcfg = model.configs['model']
    packed = [model._packed_mlp('coarse_model', True), None, None, model._packed_mlp('fine_model', True), None, None]
    kept = ops.render_keep_activations(packed, batch, model.ndc, bool(mcfg['white_bkgd']), bool(mcfg['lindisp']),
                                       mcfg['coarse_mlp']['num_samples'], mcfg['fine_mlp']['num_samples'], z_vals_fine)
    out = ops.view_sweep(packed[3], model.fine_model.abi_params(), kept['saved_acts'], kept['weights'], kept['acc'], view_dirs,
                         bool(mcfg['white_bkgd']))
    return kept, out


# ------------------------------------------------------------------------------------------------ 1. batches
def test_batches_equal_the_reference_bit_for_bit(case):
    g, dp, camera, ndc = case['g'], case['dp'], case['camera'], case['ndc']
    secondary = [dp.camera(p, i) for p, i in zip(g['secondary_poses'], g['secondary_intrinsics'])]
    batch = harness.frame_batch(camera, ndc, DEV, view_camera=case['view_cameras'][0], secondary_cameras=secondary)
    wanted = {k[len('batch_'):]: v for k, v in g.items() if k.startswith('batch_')}
    assert sorted(batch) == sorted(wanted) and 'rays_o2' in wanted and ('rays_o_ndc' in wanted) == ndc
    for key, value in wanted.items():
        assert tuple(batch[key].shape) == value.shape, key
        assert same_bits(batch[key], value), key
    for v, view_camera in enumerate(case['view_cameras']):
        assert same_bits(harness.frame_batch(camera, ndc, DEV, view_camera=view_camera)['view_dirs'], g['view_dirs'][v]), v
    # with neither argument nothing changes: today's batch, which is also create_test_data's
    plain, today = harness.frame_batch(camera, ndc, DEV), dp.create_test_data(g['pose'], intrinsic=g['intrinsic'])
    assert sorted(plain) == sorted(today) and 'rays_o2' not in plain
    for key in plain:
        assert same_bits(plain[key], today[key]), key
        if key != 'view_dirs':
            assert same_bits(plain[key], batch[key]), key
    assert not same_bits(plain['view_dirs'], batch['view_dirs'])
    part = harness.frame_batch(camera, ndc, DEV, 40, 37, view_camera=case['view_cameras'][0], secondary_cameras=secondary)
    for key in batch:
        assert same_bits(part[key], batch[key][40:]), key


# ------------------------------------------------------------------------------------------------ 2. the ordinary route
def test_ordinary_route_matches_the_reference(case):
    g, model, ndc = case['g'], case['model'], case['ndc']
    z_fine = torch.from_numpy(g['out_z_vals_fine']).to(DEV)
    for v, view_camera in enumerate(case['view_cameras']):
        model.set_random_draws({'z_vals_fine': z_fine})          # the reference's fine depths (sample_pdf's discontinuity)
        out = model(harness.frame_batch(case['camera'], ndc, DEV, view_camera=view_camera))
        colour = util.linf(out['rgb_fine'], g['out_rgb_fine'][v])
        util.observe(f'view sweep, ordinary route [{case["tag"]}, view {v}]', f'rgb_fine {colour:.2e} ({RGB_TOL:g})')
        assert colour < RGB_TOL, (v, colour)
        bad = per_ray_violation('depth_fine', out['depth_fine'], g['out_depth_fine'], g['out_acc_fine'].astype(numpy.float64), ndc)
        assert not bad.any(), (v, int(bad.sum()), util.linf(out['depth_fine'], g['out_depth_fine']), DEPTH_TOL)


# ------------------------------------------------------------------------------------------------ 3. the sweep against the reference
def test_view_sweep_matches_the_reference(case):
    g, model, ndc = case['g'], case['model'], case['ndc']
    batch = harness.frame_batch(case['camera'], ndc, DEV)
    dirs = torch.from_numpy(g['view_dirs']).to(DEV)
    kept, out = keep_and_sweep(model, batch, dirs, torch.from_numpy(g['out_z_vals_fine']).to(DEV))
    assert out.shape == (3, 77, 3) and kept['level'] == 3 and kept['num_samples'] == 192
    worst = util.linf(out, g['out_rgb_fine'])
    util.observe(f'view sweep, ops.view_sweep [{case["tag"]}]', f'rgb_fine over three view cameras {worst:.2e} ({RGB_TOL:g})')
    assert worst < RGB_TOL, worst
    assert util.linf(kept['weights'], g['out_weights_fine']) < RGB_TOL


# ------------------------------------------------------------------------------------------------ 4. the kernel's own edges
#        (MLP depth, width, views width), (coarse, fine) samples, rays, views, white_bkgd, fixture case (its cameras; ndc or not)
EDGES = [((8, 256, 128), (64, 128), 77, 3, False, 'ndc'),
         ((8, 256, 128), (20, 30), 77, 37, True, 'world'),
         ((4, 128, 64), (20, 30), 77, 37, False, 'ndc'),
         ((4, 128, 64), (64, 128), 1, 1, True, 'world'),
         ((8, 256, 128), (20, 30), 1, 3, False, 'world')]


def dense_field(configs, seed):
    """Seeded weights whose density head is scaled up and centred on sigma = 0.5: the plain initialisation is almost transparent,
    and a seed whose head happens to be negative everywhere would composite to nothing at all."""
    weights = synth.synth_state_dict(util.model_param_shapes(configs), seed, sigma_gain=60.0)
    for level in ('coarse', 'fine'):
        weights[f'{level}_model.pts_output_linear.bias'][0] = 0.5
    return {k: torch.from_numpy(v) for k, v in weights.items()}


def edge_view_cameras(dp, g, count):
    """``count`` cameras scattered around the fixture's first view camera."""
    rng = numpy.random.RandomState(count)
    cameras = []
    for _ in range(count):
        pose = g['view_poses'][0].copy()
        pose[:3, :3] = synth._rotation(*(0.4 * rng.standard_normal(3))) @ pose[:3, :3]
        pose[:3, 3] += 0.3 * rng.standard_normal(3)
        cameras.append(dp.camera(pose, g['view_intrinsics'][0]))
    return cameras


@pytest.mark.parametrize('shape, samples, n, views, white, tag', EDGES)
def test_kernel_edges(shape, samples, n, views, white, tag):
    g, _, saved, scene_configs = ref.load_case(tag)
    ndc = bool(scene_configs['data_loader']['ndc'])
    depth, width, views_width = shape
    configs = synth.with_overrides(synth.make_configs('config2'), white_bkgd=white, hip_precision='fp32',
                                   coarse_mlp=synth.mlp_config(samples[0], depth, width, views_width),
                                   fine_mlp=synth.mlp_config(samples[1], depth, width, views_width))
    configs['data_loader']['ndc'] = ndc
    model = get_model(configs, None)
    model.load_state_dict(dense_field(configs, 400 + views), strict=True)
    model = model.to(DEV).eval()
    assert harness.view_sweep_is_fast(model)
    dp = DataPreprocessor(scene_configs, 'test', model_configs=saved, device=DEV)
    camera = dp.camera(g['pose'], g['intrinsic'])
    view_cameras = edge_view_cameras(dp, g, views)
    first = 0 if n == 77 else 38
    s = samples[0] + samples[1]

    # (a) against the stack of ordinary renders, at their fine depths
    ordinary, z_fine = [], None
    for view_camera in view_cameras:
        if z_fine is not None:
            model.set_random_draws({'z_vals_fine': z_fine})
        out = model(harness.frame_batch(camera, ndc, DEV, first, n, view_camera=view_camera), retraw=True)
        z_fine = out['z_vals_fine'] if z_fine is None else z_fine
        ordinary.append(out['rgb_fine'])
    ordinary = torch.stack(ordinary)
    dirs = torch.stack([harness.view_directions(camera, view_camera, DEV, first, n) for view_camera in view_cameras])
    batch = harness.frame_batch(camera, ndc, DEV, first, n)
    kept, swept = keep_and_sweep(model, batch, dirs, z_fine)
    assert swept.shape == (views, n, 3) and kept['weights'].shape == (n, s) and torch.isfinite(swept).all()
    assert float(kept['acc'].max()) > 0.05, 'the field is transparent: the case shows nothing'
    # the tolerance: float32 against float64 restatement on the device's own inputs, times 4 (the device sums each dot product in
    # another order than numpy does)
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    inputs = (*ref.head_arrays(params, 'fine_model.'), ref.saved_feature(kept['saved_acts'].cpu().numpy(), configs['model']['fine_mlp'], n, s),
              kept['weights'].cpu().numpy(), dirs.cpu().numpy(), kept['acc'].cpu().numpy(), white)
    exact = ref.view_sweep(*inputs, dtype=numpy.float64)
    tolerance = 4 * util.linf(ref.view_sweep(*inputs, dtype=numpy.float32), exact)
    against_ordinary, against_exact = util.linf(swept, ordinary), util.linf(swept, exact)
    label = f'view sweep edges [{width}/{views_width}, {samples}, n {n}, V {views}, white {int(white)}, {tag}]'
    util.observe(label, f'against the ordinary renders {against_ordinary:.2e}, against the float64 restatement {against_exact:.2e} '
                        f'(computed tolerance {tolerance:.2e})')
    print(label, against_ordinary, against_exact, tolerance)
    assert 0 < tolerance < 1e-5
    assert against_exact <= tolerance, (against_exact, tolerance)
    assert against_ordinary <= tolerance, (against_ordinary, tolerance)
    if views > 1:
        assert util.linf(ordinary[0], ordinary[1]) > 100 * tolerance          # the view cameras do change the colour

    # (b) two identical calls: the same bits
    again = ops.view_sweep(model._packed_mlp('fine_model', True), model.fine_model.abi_params(), kept['saved_acts'], kept['weights'],
                           kept['acc'], dirs, white)
    assert same_bits(again, swept)
    # (c) a row does not depend on the other views of its call
    for v in sorted({0, views // 2, views - 1}):
        alone = ops.view_sweep(model._packed_mlp('fine_model', True), model.fine_model.abi_params(), kept['saved_acts'], kept['weights'],
                               kept['acc'], dirs[v:v + 1].contiguous(), white)
        assert same_bits(alone[0], swept[v]), v
    # (d) nor on how the frame is cut into ray blocks (with 50 samples per ray the second block starts in the middle of a tile)
    if n == 77:
        whole = harness.predict_view_sweep(model, configs, camera, view_cameras, DEV, ray_block=77)
        cut = harness.predict_view_sweep(model, configs, camera, view_cameras, DEV, ray_block=40)
        assert same_bits(whole['rgb'], cut['rgb']) and numpy.array_equal(whole['images'], cut['images'])
        for name in ('depth', 'depth_var') + (('depth_ndc', 'depth_var_ndc') if ndc else ()):
            assert same_bits(whole[name], cut[name]), name


# ------------------------------------------------------------------------------------------------ 5. frames
def test_frames_match_the_ordinary_route(case):
    model, configs, camera, ndc = case['model'], case['configs'], case['camera'], case['ndc']
    swept = harness.predict_view_sweep(model, configs, camera, case['view_cameras'], DEV)
    assert swept['images'].shape == (3, 7, 11, 3) and swept['images'].dtype == numpy.uint8
    assert swept['rgb'].shape == (3, 77, 3) and swept['rgb'].is_cuda and swept['rgb'].dtype == torch.float32
    names = ['depth', 'depth_var'] + (['depth_ndc', 'depth_var_ndc'] if ndc else [])
    assert sorted(swept) == sorted(['images', 'rgb'] + names)
    equal = {}
    for v, view_camera in enumerate(case['view_cameras']):
        frame = harness.predict_frame(model, configs, camera, DEV, view_camera=view_camera)
        levels = numpy.abs(swept['images'][v].astype(numpy.int32) - frame['image'].astype(numpy.int32)).max()
        assert levels <= 1, (v, levels)
        for name in names:
            assert swept[name].shape == (7, 11) and swept[name].dtype == numpy.float32
            worst = float(numpy.max(numpy.abs(swept[name].astype(numpy.float64) - frame[name]) / numpy.maximum(numpy.abs(frame[name]), 1.0)))
            assert worst <= DEPTH_TOL, (name, worst)
            equal[name] = equal.get(name, True) and same_bits(swept[name], frame[name])
    util.observe(f'view sweep frames [{case["tag"]}]', 'maps bit-equal to the ordinary route: ' + ', '.join(f'{k} {v}' for k, v in equal.items()))


# ------------------------------------------------------------------------------------------------ 6. the fallback route
@pytest.mark.parametrize('kind', ['f16x3', 'layered'])
def test_other_models_take_the_plain_loop(kind):
    g, base, saved, scene_configs = ref.load_case('ndc')
    if kind == 'f16x3':
        configs = synth.with_overrides(base, hip_precision='f16x3')
    else:
        configs = synth.with_overrides(base, hip_precision='fp32', coarse_mlp=synth.mlp_config(20, 4, 128, 64, views_depth=2),
                                       fine_mlp=synth.mlp_config(30, 4, 128, 64, views_depth=2))
    model = get_model(configs, None)
    model.load_state_dict(dense_field(configs, 77), strict=True)
    model = model.to(DEV).eval()
    assert not harness.view_sweep_is_fast(model)
    dp = DataPreprocessor(scene_configs, 'test', model_configs=saved, device=DEV)
    camera = dp.camera(g['pose'], g['intrinsic'])
    view_cameras = [dp.camera(p, i) for p, i in zip(g['view_poses'][:2], g['view_intrinsics'][:2])]
    swept = harness.predict_view_sweep(model, configs, camera, view_cameras, DEV)
    assert swept['images'].shape == (2, 7, 11, 3) and swept['rgb'].shape == (2, 77, 3)
    for v, view_camera in enumerate(view_cameras):
        frame = harness.predict_frame(model, configs, camera, DEV, view_camera=view_camera)
        assert numpy.array_equal(swept['images'][v], frame['image'])
        rendered = harness.render_frame(model, camera, True, DEV, ['rgb_fine'], view_camera=view_camera)['rgb_fine']
        assert same_bits(swept['rgb'][v], rendered)
        for name in ('depth', 'depth_var', 'depth_ndc', 'depth_var_ndc'):
            assert same_bits(swept[name], frame[name]), name
    assert not numpy.array_equal(swept['rgb'][0].cpu().numpy(), swept['rgb'][1].cpu().numpy())


# ------------------------------------------------------------------------------------------------ 7. files
def test_static_camera_frames_are_written_under_the_reference_names(case, tmp_path):
    g, model, dp = case['g'], case['model'], case['dp']
    extrinsics = numpy.concatenate([g['pose'][None], g['view_poses']])          # (4,4,4) raw poses
    result = harness.save_static_camera_frames(model, case['configs'], dp, extrinsics, tmp_path, DEV)
    written = sorted(os.path.relpath(os.path.join(root, name), tmp_path) for root, _, names in os.walk(tmp_path) for name in names)
    assert written == [os.path.join('predicted_frames', f'{i:04}.png') for i in range(3)]
    assert result['images'].shape == (3, 7, 11, 3)
    for i, name in enumerate(written):
        with open(os.path.join(tmp_path, name), 'rb') as f:
            assert numpy.array_equal(validation_reference.decode_png(f.read()), result['images'][i]), name
    assert not numpy.array_equal(result['images'][0], result['images'][1])
