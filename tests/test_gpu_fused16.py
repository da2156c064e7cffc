"""The fused per-ray-tile render in the single-product 16-bit modes (render_fused_m16_kernel, csrc/render_fused.hip;
configs['model']['hip_fused_render']): f16 / bf16 / f16s8 / bf16s8 renders of a plain coarse + fine 8 x 256 model in ONE launch
around the body of the m16 forward.  Same device functions in the same order as the six-launch path, so every output must be
BIT-IDENTICAL in each precision; calls outside its scope take the six-launch path."""
import numpy
import pytest
import torch

from simplenerf_amd import harness, ops, synth
from simplenerf_amd.models.ModelFactory import get_model
from tests import util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PRECISIONS = ['f16', 'bf16', 'f16s8', 'bf16s8']
SAMPLES = {'config2': (64, 128), 'headline': (128, 128)}


def pair(kind, precision, binding='torch_ext', coarse_samples=None, state=None, train=False, **overrides):
    """(six-launch model, fused model) with the same synthetic weights (or `state`)"""
    models = []
    for fused in (False, True):
        cfg = synth.with_overrides(synth.make_configs(kind), hip_precision=precision, hip_fused_render=fused,
                                   hip_host_binding=binding, **overrides)
        if coarse_samples:
            cfg['model']['coarse_mlp']['num_samples'] = coarse_samples
        model = get_model(cfg, None)
        if state is None:
            shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
            state = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 7, 200.0, 8.0).items()}
        model.load_state_dict(state)
        models.append(model.to(DEV).train(train))
    return models


def launches_of(model, batch):
    """MLP-forward launches the library times for one call of the model (1 = the fused kernel, 2 = coarse + fine)"""
    ops.profile_enable(16)
    with torch.no_grad():
        model(batch)
    torch.cuda.synchronize()
    ms, samples = ops.profile_collect(ops.PROFILE_MLP_FORWARD)
    ops.profile_enable(0)
    return len(ms), sum(samples)


def assert_identical(got, want):
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert torch.equal(got[k], v), (k, util.linf(got[k], v))


@pytest.mark.parametrize('count', [1, 3, 1000, 1027])
@pytest.mark.parametrize('kind', ['config2', 'headline'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_fused16_render_is_bit_identical_to_the_six_launch_path(precision, kind, count):
    plain, fused = pair(kind, precision)
    batch = harness.frame_batch(synth.camera('fern', 0), True, DEV, 190000, count)
    ops.range_status(clear=True)
    with torch.no_grad():
        want = plain(batch, retraw=True)
        got = fused(batch, retraw=True)
    torch.cuda.synchronize()
    assert ops.range_status() == 0
    assert_identical(got, want)
    assert float(want['acc_fine'].mean()) > 0.05
    s_c, s_f = SAMPLES[kind]
    assert launches_of(plain, batch) == (2, count * (2 * s_c + s_f))
    assert launches_of(fused, batch) == (1, count * (2 * s_c + s_f))


@pytest.mark.parametrize('precision', ['bf16', 'f16'])
def test_fused16_render_through_the_ctypes_binding(precision):
    plain, fused = pair('headline', precision, binding='ctypes')
    batch = harness.frame_batch(synth.camera('fern', 0), True, DEV, 190000, 517)
    with torch.no_grad():
        want = plain(batch, retraw=True)
        got = fused(batch, retraw=True)
    assert_identical(got, want)
    assert launches_of(fused, batch) == (1, 517 * (2 * 128 + 128))


@pytest.mark.parametrize('precision', ['bf16', 'f16'])
def test_fused16_render_of_world_rays_and_white_background(precision):
    """non-NDC rays (headline_world) and model.white_bkgd"""
    plain, fused = pair('headline_world', precision, white_bkgd=True)
    batch = {k: torch.from_numpy(v).to(DEV) for k, v in synth.random_world_rays(300, seed=5).items()}
    with torch.no_grad():
        want, got = plain(batch), fused(batch)
    assert_identical(got, want)
    assert launches_of(fused, batch)[0] == 1


@pytest.mark.parametrize('precision', ['bf16', 'f16'])
def test_fused16_full_frame_equals_the_six_launch_frame(precision):
    """harness.predict_frame (65 536-ray blocks) of the 504 x 378 fern frame: the display outputs are identical."""
    plain, fused = pair('config2', precision)
    cam = synth.camera('fern', 0, downscale=2)
    cfg = synth.with_overrides(synth.make_configs('config2'), hip_precision=precision)
    want = harness.predict_frame(plain, cfg, cam, torch.device(DEV))
    got = harness.predict_frame(fused, cfg, cam, torch.device(DEV))
    assert sorted(got) == sorted(want) and all(numpy.array_equal(got[k], want[k]) for k in want)


def test_fused16_render_leaving_the_fp16_range_is_reported_like_the_six_launch_render():
    """A hidden unit driven past 65 504 (as tests/test_gpu_f16.py does): the fused f16 render raises the device's range flag and
    the NEXT fp16-mode call raises Fp16RangeError, exactly as the six-launch render does.  bf16 has no range limit: the same
    weights render finite, and fused equals six-launch."""
    plain, fused = pair('config2', 'f16')
    batch = harness.frame_batch(synth.camera('fern', 0), True, DEV, 200000, 64)
    with torch.no_grad():
        for m in (plain, fused):
            m.coarse_model.pts_linears[2].bias[17] = 1.0e5
    for model in (plain, fused):
        ops.range_status(clear=True)
        with torch.no_grad():
            model(batch)                       # enqueued before the flag can be seen: no error from this call
        torch.cuda.synchronize()
        assert ops.range_status() & ops.RANGE_ACTIVATION
        with pytest.raises(ops.Fp16RangeError, match='fp16 range'):
            with torch.no_grad():
                model(batch)
        assert ops.range_status() == 0         # reported once; the refused call enqueued nothing
    assert launches_of(fused, batch)[0] == 1
    ops.range_status(clear=True)
    state = plain.state_dict()
    plain16, fused16 = pair('config2', 'bf16', state=state)
    with torch.no_grad():
        want, got = plain16(batch), fused16(batch)
    torch.cuda.synchronize()
    assert ops.range_status() == 0
    assert all(torch.isfinite(v).all() for v in want.values())
    assert_identical(got, want)


def test_fused16_calls_outside_the_kernels_scope_take_the_six_launch_path():
    """A 4 x 128 model in f16, a 48-coarse-sample model in bf16 and a training-mode forward in bf16 run stage by stage: same
    results as with the flag off, two MLP launches, no error."""
    batch = harness.frame_batch(synth.camera('fern', 0), True, DEV, 190000, 64)
    for what, (plain, fused) in (('4 x 128, f16', pair_narrow('f16')), ('48 coarse samples, bf16', pair('config2', 'bf16', coarse_samples=48))):
        with torch.no_grad():
            want, got = plain(batch), fused(batch)
        assert_identical(got, want)
        assert launches_of(plain, batch)[0] == 2 and launches_of(fused, batch)[0] == 2, what
    # training mode: the forward keeps its activations for the backward -- never fused (both models' first training call: the
    # same draws)
    plain, fused = pair('config2', 'bf16', train=True)
    outs = []
    for model in (plain, fused):
        out = model(batch)
        out['rgb_fine'].sum().backward()
        outs.append((out, [p.grad.clone() for p in model.fine_model.parameters()]))
    (want, want_grads), (got, got_grads) = outs
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert all(torch.isfinite(g).all() for g in got_grads)
    assert all(torch.equal(g, w) for g, w in zip(got_grads, want_grads))
    assert launches_of(fused, batch)[0] == 2


def pair_narrow(precision):
    """config2 with 4 x 128 coarse and fine MLPs (views width 64): the 16-bit modes render it on mlp_forward_f16.hip"""
    models = []
    state = None
    for fused in (False, True):
        cfg = synth.with_overrides(synth.make_configs('config2'), hip_precision=precision, hip_fused_render=fused)
        for level in ('coarse_mlp', 'fine_mlp'):
            cfg['model'][level].update(synth.mlp_config(cfg['model'][level]['num_samples'], depth=4, width=128, views_width=64))
        model = get_model(cfg, None)
        if state is None:
            shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
            state = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 7, 200.0, 8.0).items()}
        model.load_state_dict(state)
        models.append(model.to(DEV).eval())
    return models
