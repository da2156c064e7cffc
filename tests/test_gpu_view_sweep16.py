"""The view sweep of the 16-bit modes on a real MI355X (``snerf_view_sweep_half``, csrc/view_sweep16.hip): which models take the
one-trunk-pass route, the kernel against a float64 restatement on the device's own operands (tests/view_sweep16_reference.py decodes
the saved pieces by the header's layout text) and against the keep-activations render of the same kernel family at a tolerance
computed here, its edges (samples of several rays in one 32-sample block, a partial last block, a block count that is no multiple
of the waves per workgroup, one ray, 37 views, white background, a coarse-only model), determinism, independence of the views and of
the ray blocks, the depth maps, the reference's colours at the modes' own bars, and the 8-bit modes bit for bit."""
import numpy
import pytest
import torch

from simplenerf_amd import harness, ops, synth
from simplenerf_amd.data_preprocessors.DataPreprocessor01 import DataPreprocessor
from simplenerf_amd.models.ModelFactory import get_model
from tests import util
from tests import view_sweep16_reference as ref16
from tests import view_sweep_reference as ref
from tests.test_gpu_view_sweep import edge_view_cameras, same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODES = ('f16', 'bf16')
SHAPE = (2, 256, 128)           # trunk depth, width, views width of every MLP below
# the reference's colours: the bars the modes' own renders are held to (tests/test_gpu_f16.py test_f16_render_close_to_fp32,
# tests/test_gpu_bf16.py test_bf16_render_close_to_fp32)
REFERENCE_RGB_TOL = {'f16': 1e-3, 'bf16': 4e-3}

#        (coarse, fine) samples (fine 0: a coarse-only model), first ray, rays, views, fixture case (its cameras; 'world' is white)
CASES = {'straddling': ((20, 30), 0, 77, 3, 'ndc'),          # blocks straddle rays, a partial last block, 121 blocks = 30 x 4 + 1
         'one_block': ((3, 2), 38, 1, 1, 'world'),           # a single partial block (the resampling needs three coarse samples)
         'many_views': ((12, 20), 0, 64, 37, 'world'),       # whole blocks only, white background
         'coarse_only': ((40, 0), 0, 77, 3, 'ndc')}          # the displayed level is 0


def dense_field(configs, seed):
    """tests/test_gpu_view_sweep.dense_field for models with or without a fine MLP."""
    weights = synth.synth_state_dict(util.model_param_shapes(configs), seed, sigma_gain=60.0)
    for key in weights:
        if key.endswith('_model.pts_output_linear.bias'):
            weights[key][0] = 0.5
    return {k: torch.from_numpy(v) for k, v in weights.items()}


def make_model(samples, tag, precision):
    g, _, saved, scene_configs = ref.load_case(tag)
    ndc = bool(scene_configs['data_loader']['ndc'])
    configs = synth.with_overrides(synth.make_configs('config2'), white_bkgd=bool(scene_configs['model']['white_bkgd']), hip_precision=precision,
                                   coarse_mlp=synth.mlp_config(samples[0], *SHAPE), fine_mlp=synth.mlp_config(samples[1], *SHAPE))
    if not samples[1]:
        del configs['model']['fine_mlp']
    configs['data_loader']['ndc'] = ndc
    model = get_model(configs, None)
    model.load_state_dict(dense_field(configs, 416), strict=True)
    return model.to(DEV).eval(), configs


def keep(model, batch):
    """A keep-activations render of ``batch`` at the model's precision -> (packed MLPs, the displayed level's module, kept)."""
    mcfg = model.configs['model']
    levels = harness._sweep_levels(model)
    packed = [None] * 6
    for level, _ in levels:
        packed[level] = model._packed_mlp('coarse_model' if level == 0 else 'fine_model', True)
    kept = ops.render_keep_activations(packed, batch, model.ndc, bool(mcfg['white_bkgd']), bool(mcfg['lindisp']),
                                       mcfg['coarse_mlp']['num_samples'], mcfg['fine_mlp']['num_samples'] if len(levels) == 2 else 0,
                                       precision=model.precision)
    assert kept['level'] == levels[-1][0]
    return packed, levels[-1][1], kept


_built = {}


def built(name, mode):
    """One case in one mode, computed once and shared by the tests below (nothing in it is changed afterwards): the model, the
    cameras, the kept render, the settled view directions, the sweep, the two restatements and the tolerance."""
    if (name, mode) in _built:
        return _built[name, mode]
    samples, first, n, views, tag = CASES[name]
    model, configs = make_model(samples, tag, mode)
    g, _, saved, scene_configs = ref.load_case(tag)
    dp = DataPreprocessor(scene_configs, 'test', model_configs=saved, device=DEV)
    camera = dp.camera(g['pose'], g['intrinsic'])
    view_cameras = edge_view_cameras(dp, g, views)
    degree = configs['model']['coarse_mlp']['views_positional_encoding_degree']
    dirs = torch.stack([harness.view_directions(camera, view_camera, DEV, first, n) for view_camera in view_cameras])
    dirs = torch.from_numpy(ref16.settled_directions(dirs.cpu().numpy(), degree, mode)).to(DEV)
    batch = harness.frame_batch(camera, model.ndc, DEV, first, n)
    packed, module, kept = keep(model, batch)
    level = kept['level']
    white = bool(configs['model']['white_bkgd'])
    sweep = lambda d: ops.view_sweep_half(packed[level], module.abi_params(), kept['saved_acts'], kept['weights'], kept['acc'], d, white,
                                          model.precision)
    swept = sweep(dirs)
    s = kept['num_samples']
    assert s == sum(samples) and swept.shape == (views, n, 3) and kept['weights'].shape == (n, s) and bool(torch.isfinite(swept).all())
    assert float(kept['acc'].max()) > 0.05, 'the field is transparent: the case shows nothing'
    prefix = 'fine_model.' if level == 3 else 'coarse_model.'
    mlp_cfg = configs['model']['fine_mlp' if level == 3 else 'coarse_mlp']
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    feature = ref16.saved_feature(kept['saved_acts'].cpu().numpy(), mlp_cfg, n, s, mode)
    inputs = (*ref.head_arrays(params, prefix), feature, kept['weights'].cpu().numpy(), dirs.cpu().numpy(), kept['acc'].cpu().numpy(), white)
    exact = ref16.view_sweep(*inputs, mode=mode, dtype=numpy.float64)
    # the tolerance: float32 against float64 restatement on the device's own operands, times 4 (the device sums each dot product in
    # another order than numpy does)
    tolerance = 4 * util.linf(ref16.view_sweep(*inputs, mode=mode, dtype=numpy.float32), exact)
    _built[name, mode] = dict(model=model, configs=configs, camera=camera, view_cameras=view_cameras, dirs=dirs, batch=batch, kept=kept,
                              sweep=sweep, swept=swept, exact=exact, tolerance=tolerance, feature=feature, white=white, n=n, views=views,
                              first=first, label=f'view sweep [{mode}, {name}: {samples}, n {n}, V {views}, white {int(white)}]')
    return _built[name, mode]


# ------------------------------------------------------------------------------------------------ 1. which models are fast
@pytest.mark.parametrize('precision, fast', [('f16', True), ('bf16', True), ('f16s8', True), ('bf16s8', True), ('f16x3', False)])
def test_which_precisions_take_the_one_trunk_pass_route(precision, fast):
    model, _ = make_model((20, 30), 'ndc', precision)
    assert harness.view_sweep_is_fast(model) is fast


def test_visibility_and_layered_shapes_stay_on_the_plain_loop():
    _, base, _, _ = ref.load_case('ndc')
    for mlp in (synth.mlp_config(20, 4, 128, 64, views_depth=2), synth.mlp_config(20, 2, 256, 128, predict_visibility=True)):
        model = get_model(synth.with_overrides(base, hip_precision='bf16', coarse_mlp=mlp, fine_mlp=dict(mlp, num_samples=30)), None)
        assert not harness.view_sweep_is_fast(model)


# ------------------------------------------------------------------------------------------------ 2. the float64 restatement
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(CASES))
def test_sweep_against_the_float64_restatement(name, mode):
    c = built(name, mode)
    worst = util.linf(c['swept'], c['exact'])
    util.observe(c['label'], f'against the float64 restatement {worst:.2e} (computed tolerance {c["tolerance"]:.2e})')
    print(c['label'], worst, c['tolerance'])
    assert 0 < c['tolerance'] < 1e-5
    assert worst <= c['tolerance'], (worst, c['tolerance'])
    assert numpy.abs(c['feature']).max() > 0.1          # the decoded pieces are no zeros
    if c['views'] > 1:
        assert util.linf(c['swept'][0], c['swept'][1]) > 100 * c['tolerance']          # the view cameras do change the colour


# ------------------------------------------------------------------------------------------------ 3. the same kernel family
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(CASES))
def test_sweep_against_the_keep_activations_render(name, mode):
    """The storing forward with view camera v's directions on the rays: the same features, the same rounded operands in the views
    layer; its colour differs from the sweep's in the order of the fp32 sums only."""
    c = built(name, mode)
    worst = 0.0
    for v in sorted({0, c['views'] // 2, c['views'] - 1}):
        batch = dict(c['batch'], view_dirs=c['dirs'][v].contiguous())
        _, _, rendered = keep(c['model'], batch)
        assert same_bits(rendered['weights'], c['kept']['weights'])          # (the density does not see the view direction)
        worst = max(worst, util.linf(c['swept'][v], rendered['outputs']['rgb']))
    util.observe(c['label'], f'against the keep-activations render {worst:.2e} (computed tolerance {c["tolerance"]:.2e})')
    print(c['label'], worst, c['tolerance'])
    assert worst <= c['tolerance'], (worst, c['tolerance'])


# ------------------------------------------------------------------------------------------------ 4. bit for bit
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(CASES))
def test_two_calls_agree_and_a_view_does_not_depend_on_the_others(name, mode):
    c = built(name, mode)
    assert same_bits(c['sweep'](c['dirs']), c['swept'])
    for v in sorted({0, c['views'] // 2, c['views'] - 1}):
        alone = c['sweep'](c['dirs'][v:v + 1].contiguous())
        assert same_bits(alone[0], c['swept'][v]), v


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['straddling', 'coarse_only'])
def test_frames_do_not_depend_on_the_ray_blocks_and_carry_the_kept_render_maps(name, mode):
    """With 50 (40) samples per ray the second block of 40 rays starts in the middle of a 32-sample tile."""
    c = built(name, mode)
    model, configs, camera, view_cameras = c['model'], c['configs'], c['camera'], c['view_cameras']
    assert harness.view_sweep_is_fast(model)
    whole = harness.predict_view_sweep(model, configs, camera, view_cameras, DEV, ray_block=77)
    cut = harness.predict_view_sweep(model, configs, camera, view_cameras, DEV, ray_block=40)
    default = harness.predict_view_sweep(model, configs, camera, view_cameras, DEV)
    assert whole['rgb'].shape == (3, 77, 3) and whole['images'].shape == (3, 7, 11, 3)
    assert same_bits(whole['rgb'], cut['rgb']) and numpy.array_equal(whole['images'], cut['images'])
    assert same_bits(whole['rgb'], default['rgb'])
    names = ('depth', 'depth_var') + (('depth_ndc', 'depth_var_ndc') if model.ndc else ())
    _, module, kept = keep(model, harness.frame_batch(camera, model.ndc, DEV))
    for key in names:
        assert same_bits(whole[key], cut[key]), key
        assert same_bits(whole[key].reshape(-1), ops.to_display(None, kept['outputs'][key], colour=False)[1]), key
    # the frame is the sweep of the cameras' own (unsettled) directions
    dirs = torch.stack([harness.view_directions(camera, view_camera, DEV) for view_camera in view_cameras])
    packed =model._packed_mlp('fine_model' if kept['level'] == 3 else 'coarse_model', True)
    direct = ops.view_sweep_half(packed, module.abi_params(), kept['saved_acts'], kept['weights'], kept['acc'], dirs, c['white'], model.precision)
    assert same_bits(whole['rgb'], direct)


# ------------------------------------------------------------------------------------------------ 5. the reference's colours
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('tag', ref.CASES)
def test_frames_match_the_reference_at_the_colour_bar_of_the_mode(tag, mode):
    """The fixture's model is 8 x 256 / 128 with sigma_pe_degree -1 and no visibility: a shape the 16-bit route accepts."""
    g, configs, saved, scene_configs = ref.load_case(tag)
    model = get_model(synth.with_overrides(configs, hip_precision=mode), None)
    model.load_state_dict(util.golden_params(configs, g), strict=True)
    model = model.to(DEV).eval()
    assert harness.view_sweep_is_fast(model)
    dp = DataPreprocessor(scene_configs, 'test', model_configs=saved, device=DEV)
    camera = dp.camera(g['pose'], g['intrinsic'])
    view_cameras = [dp.camera(p, i) for p, i in zip(g['view_poses'], g['view_intrinsics'])]
    swept = harness.predict_view_sweep(model, model.configs, camera, view_cameras, DEV)
    assert swept['rgb'].shape == (3, 77, 3) and swept['images'].shape == (3, 7, 11, 3) and swept['images'].dtype == numpy.uint8
    worst = util.linf(swept['rgb'], g['out_rgb_fine'])
    util.observe(f'view sweep, reference colours [{mode}, {tag}]', f'rgb_fine over three view cameras {worst:.2e} ({REFERENCE_RGB_TOL[mode]:g})')
    print(tag, mode, worst)
    assert worst < REFERENCE_RGB_TOL[mode], worst
    assert util.linf(swept['rgb'][0], swept['rgb'][1]) > 1e-2          # the view cameras do change the colour


# ------------------------------------------------------------------------------------------------ 6. the 8-bit modes
@pytest.mark.parametrize('mode', MODES)
def test_the_8_bit_modes_give_the_base_mode_s_frames_bit_for_bit(mode):
    c = built('straddling', mode)
    base = harness.predict_view_sweep(c['model'], c['configs'], c['camera'], c['view_cameras'], DEV)
    model, configs = make_model(CASES['straddling'][0], CASES['straddling'][4], mode + 's8')
    assert model.precision == ops.PRECISIONS[mode + 's8'] and harness.view_sweep_is_fast(model)
    other = harness.predict_view_sweep(model, configs, c['camera'], c['view_cameras'], DEV)
    assert sorted(other) == sorted(base)
    assert same_bits(other['rgb'], base['rgb']) and numpy.array_equal(other['images'], base['images'])
    for key in base:
        if key not in ('rgb', 'images'):
            assert same_bits(other[key], base[key]), key
