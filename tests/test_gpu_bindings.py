"""The two host bindings of the one-call render ops -- torch.ops.snerf.render (TORCH_LIBRARY extension with a C++ autograd
node, csrc_torch/snerf_torch.cpp) and ops.RenderCall (ctypes) -- drive the same two C-ABI entry points: outputs, parameter
gradients, accumulation into existing gradients and the returned-gradient mode must agree BIT FOR BIT."""
import gc

import pytest
import torch

from simplenerf_amd import harness, ops, synth
from simplenerf_amd.models.ModelFactory import get_model
from tests import util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def make(kind, binding, precision='fp32', **overrides):
    cfg = synth.with_overrides(synth.make_configs(kind), hip_precision=precision, hip_host_binding=binding, **overrides)
    model = get_model(cfg, None)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 7, 200.0, 8.0).items()})
    return model.to(DEV)


@pytest.mark.parametrize('kind', ['config1', 'config2', 'headline_world'])
@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
def test_eval_outputs_are_identical(kind, precision):
    models = {b: make(kind, b, precision).eval() for b in ('torch_ext', 'ctypes')}
    if kind == 'config1':
        batch = {k: torch.from_numpy(v).to(DEV) for k, v in synth.random_world_rays(301, seed=4).items()}
    else:
        cam = synth.camera('fern', 0)
        batch = harness.frame_batch(cam, kind == 'config2', DEV, 300000, 301)
    with torch.no_grad():
        for retraw in (False, True):
            a, b = models['torch_ext'](batch, retraw=retraw), models['ctypes'](batch, retraw=retraw)
            assert list(a.keys()) == list(b.keys())
            for k in a:
                assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, retraw)
        # the fine-depth override comes back as z_vals_fine through both
        if kind != 'config1':
            z = b['z_vals_fine'].clone()
            for m in models.values():
                m.set_random_draws({'z_vals_fine': z})
            a, b = models['torch_ext'](batch, retraw=True), models['ctypes'](batch, retraw=True)
            assert torch.equal(a['z_vals_fine'], z) and all(torch.equal(a[k], b[k]) for k in a)


def test_predicted_visibility_with_secondary_views_is_identical():
    """The route with the most layout rules -- predict_visibility levels, two secondary views (scratch view directions, weights
    carved only for visibility2, visibility2 among the per-ray outputs), NDC, every per-sample output -- through both bindings, with
    and without injected fine depths."""
    from tests.test_gpu_model import build
    from tests.test_oracle_golden import visibility_case
    g, cfg, batch = visibility_case('ndc_eval')
    models = {b: build(synth.with_overrides(cfg, hip_host_binding=b), g).eval() for b in ('torch_ext', 'ctypes')}
    batch = {k: v.to(DEV) if isinstance(v, torch.Tensor) else v for k, v in batch.items()}
    with torch.no_grad():
        for z_fine in (None, torch.from_numpy(g['out_z_vals_fine'])):
            for retraw in (True, False):          # (without retraw the weights are carved but not returned)
                if z_fine is not None:
                    for m in models.values():
                        m.set_random_draws({'z_vals_fine': z_fine})
                a, b = (models[name](batch, retraw=retraw, sec_views_vis=True) for name in ('torch_ext', 'ctypes'))
                assert list(a.keys()) == list(b.keys()) and ('weights_fine' in a) == retraw
                assert {'visibility2_coarse', 'visibility2_fine'} <= set(a) and (not retraw or 'raw_visibility2_fine' in a)
                for k in a:
                    assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, retraw, z_fine is not None)
                if z_fine is not None and retraw:
                    assert torch.equal(a['z_vals_fine'].cpu(), z_fine)


# config 3 in training mode (levels 0-3, NDC, 64 + 128 samples, every per-sample output): floats per ray from the start of its pool
# of every output, worked out by hand from the order the pools are carved in -- per level rgb, acc, depth, depth_var, depth_ndc,
# depth_var_ndc in the per-ray pool; z_vals_coarse, z_vals_fine, then per level alpha, visibility, weights, sigma, raw_rgb
CONFIG3_PER_RAY = {'rgb': 0, 'acc': 3, 'depth': 4, 'depth_var': 5, 'depth_ndc': 6, 'depth_var_ndc': 7}         # + 8 per level
CONFIG3_PER_SAMPLE = {
    'z_vals_coarse': 0, 'z_vals_fine': 64,
    'alpha_coarse': 256, 'visibility_coarse': 320, 'weights_coarse': 384, 'raw_sigma_coarse': 448, 'raw_rgb_coarse': 512,
    'points_augmentation_alpha_coarse': 704, 'points_augmentation_visibility_coarse': 768, 'points_augmentation_weights_coarse': 832,
    'points_augmentation_raw_sigma_coarse': 896, 'points_augmentation_raw_rgb_coarse': 960,
    'views_augmentation_alpha_coarse': 1152, 'views_augmentation_visibility_coarse': 1216, 'views_augmentation_weights_coarse': 1280,
    'views_augmentation_raw_sigma_coarse': 1344, 'views_augmentation_raw_rgb_coarse': 1408,
    'alpha_fine': 1600, 'visibility_fine': 1792, 'weights_fine': 1984, 'raw_sigma_fine': 2176, 'raw_rgb_fine': 2368}


@pytest.mark.parametrize('binding', ['torch_ext', 'ctypes'])
def test_outputs_lie_where_the_pools_were_always_carved(binding):
    """The memory layout inside the two pools: every output of a training-mode config 3 call starts n x (the hand-derived offset)
    floats into its pool, z_vals_coarse at the base of the per-sample pool and rgb_coarse at the base of the per-ray pool."""
    n = 37
    model = make('config3', binding).train()
    batch = harness.frame_batch(synth.camera('fern', 0), True, DEV, 250000, n)
    batch['iter_num'] = 0
    out = model(batch)
    expected = dict(CONFIG3_PER_SAMPLE)
    levels = ('{}_coarse', 'points_augmentation_{}_coarse', 'views_augmentation_{}_coarse', '{}_fine')
    per_ray = [pattern.format(k) for pattern in levels for k in CONFIG3_PER_RAY]
    expected.update({pattern.format(k): 8 * l + at for l, pattern in enumerate(levels) for k, at in CONFIG3_PER_RAY.items()})
    views = {k: v for k, v in out.items() if 'rgb_view_' not in k}                 # (those name raw_rgb a second time)
    assert set(views) == set(expected), set(views) ^ set(expected)
    for k, v in views.items():
        assert v.is_contiguous() and v.storage_offset() == n * expected[k], (k, v.storage_offset(), n * expected[k])
        pool = out['rgb_coarse'] if k in per_ray else out['z_vals_coarse']
        assert v.untyped_storage().data_ptr() == pool.untyped_storage().data_ptr(), k
    assert out['z_vals_coarse'].data_ptr() == out['z_vals_coarse'].untyped_storage().data_ptr()
    assert out['rgb_coarse'].data_ptr() == out['rgb_coarse'].untyped_storage().data_ptr()
    assert out['z_vals_coarse'].untyped_storage().nbytes() == 4 * n * 2944 and out['rgb_coarse'].untyped_storage().nbytes() == 4 * n * 32


@pytest.mark.parametrize('binding', ['torch_ext', 'ctypes'])
def test_a_call_without_rays_returns_empty_outputs_of_the_right_shapes(binding):
    model = make('config2', binding).eval()
    cam = synth.camera('fern', 0)
    with torch.no_grad():
        full, out = (model(harness.frame_batch(cam, True, DEV, 1000, n), retraw=True) for n in (4, 0))
    assert list(out.keys()) == list(full.keys())
    for k in out:
        assert tuple(out[k].shape) == (0,) + tuple(full[k].shape[1:]), k


@pytest.mark.parametrize('precision', ['fp32', 'f16'])
def test_training_outputs_and_gradients_are_identical(precision):
    """config 3 (four MLPs, device draws keyed by iteration and row): two backward passes (overwrite, then accumulate into the
    existing .grad), every parameter."""
    models = {b: make('config3', b, precision).train() for b in ('torch_ext', 'ctypes')}
    cam = synth.camera('fern', 0)
    grads = {}
    for name, model in models.items():
        for it in (3, 4):
            batch = harness.frame_batch(cam, True, DEV, 250000 + 100 * it, 130)
            batch['iter_num'] = it
            out = model(batch)
            assert out['rgb_fine'].requires_grad and not out['alpha_fine'].requires_grad and not out['z_vals_fine'].requires_grad
            util.grad_loss(out).backward()
        grads[name] = {k: p.grad.clone() for k, p in model.named_parameters()}
        grads[name + '/out'] = {k: v.detach().clone() for k, v in out.items()}
    for k in grads['ctypes']:
        assert torch.equal(grads['torch_ext'][k], grads['ctypes'][k]), k
    for k in grads['ctypes/out']:
        assert torch.equal(grads['torch_ext/out'][k], grads['ctypes/out'][k]), k


def test_returned_gradient_mode_and_autograd_grad():
    """hip_return_param_grads: the node hands the parameter gradients back to autograd (torch.autograd.grad works)."""
    cam = synth.camera('fern', 0)
    batch = harness.frame_batch(cam, True, DEV, 123456, 64)
    batch['iter_num'] = 0
    results = {}
    for binding in ('torch_ext', 'ctypes'):
        model = make('config3', binding, hip_return_param_grads=True).train()
        out = model(batch)
        params = list(model.parameters())
        got = torch.autograd.grad(util.grad_loss(out), params, allow_unused=True)
        assert all(p.grad is None for p in params)
        results[binding] = got
    for a, b in zip(results['torch_ext'], results['ctypes']):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))


def test_extension_frees_its_memory_without_the_cycle_collector():
    """The C++ node owns the call object (pools, saved activations) and must die with the outputs -- no reference cycle."""
    model = make('config3', 'torch_ext').train()
    cam = synth.camera('fern', 0)
    gc.disable()
    try:
        torch.cuda.synchronize()
        base = None
        for it in range(12):
            batch = harness.frame_batch(cam, True, DEV, 200000, 512)
            batch['iter_num'] = it
            out = model(batch)
            if it % 2 == 0:
                util.grad_loss(out).backward()      # (odd iterations drop the graph without a backward)
            del out
            torch.cuda.synchronize()
            used = torch.cuda.memory_allocated()
            if it == 3:
                base = used
            if it > 3:
                assert used <= base * 1.05 + (1 << 20), (it, used, base)
    finally:
        gc.enable()


def test_extension_errors_are_runtime_errors():
    model = make('config2', 'torch_ext').eval()
    cam = synth.camera('fern', 0)
    batch = harness.frame_batch(cam, True, DEV, 1000, 16)
    bad = dict(batch, rays_d=batch['rays_d'][:8])
    with pytest.raises(RuntimeError, match='rays_d'):
        with torch.no_grad():
            model(bad)
    bad = dict(batch, near_ndc=batch['near_ndc'].double())
    with pytest.raises(RuntimeError, match='float32'):
        with torch.no_grad():
            model(bad)
    del batch['view_dirs']
    with pytest.raises(RuntimeError, match='view_dirs'):
        with torch.no_grad():
            model(batch)
