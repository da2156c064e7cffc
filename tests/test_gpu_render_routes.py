"""Every render route on the options and rays no other test runs: the narrow (4 x 128) fp32 fused kernels, ``lindisp`` with a
fine level (resampling from disparity-spaced strata), and the stratified jitter ``t_rand`` and inverse-CDF draws ``u`` inside
both fused kernels -- a ``train()`` model under ``no_grad`` keeps no activations, so that call fuses and takes stage 1's jitter
branch and resample_wave's unsorted-samples merge on the LDS-resident tile.

Gates of every case (7 rays: full ray groups and a tail group in both kernels):
  G1  fused == six-launch on every key (retraw), bit for bit; one MLP launch against two with the expected sample counts -- the
      proof that the fused kernel ran and the call did not fall back; fp16: the range flag stays clear;
  G2  z_vals_coarse == the oracle's, bit for bit (lindisp, jitter);
  G3  z_vals_fine == oracle.resample_depths evaluated on the CPU from the device's own coarse depths and weights, bit for bit
      (check_resample's contract inside each route and precision);
  G4  fp32: against oracle.render -- no ray of a coarse-level key over per_ray_violation's bounds, and none of a fine-level
      key once the six-launch model is given the oracle's fine depths (the intervention of
      test_fine_pass_on_reference_samples: seven rays are too few for outlier fractions)."""
import numpy
import pytest
import torch

from oracle import nerf_oracle as oracle
from simplenerf_amd import harness, ops, synth
from tests import render_cases as rc
from tests import util
from tests.test_gpu_fused import launches_of
from tests.test_gpu_model import per_ray_violation

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RAYS = 7


def rays_of(kind, count, seed=5):
    """config2: NDC rays of the fern camera; otherwise world rays"""
    if kind == 'config2':
        return harness.frame_batch(synth.camera('fern', 0), True, DEV, 190000, count)
    return {k: torch.from_numpy(v).to(DEV) for k, v in synth.random_world_rays(count, seed=seed).items()}


def draws_for(model, count, seed):
    """t_rand and u as the reference's torch.rand would hand them over (uniform in [0, 1))"""
    m = model.configs['model']
    gen = torch.Generator().manual_seed(seed)
    return {'t_rand': torch.rand((count, m['coarse_mlp']['num_samples']), generator=gen),
            'u': torch.rand((count, m['fine_mlp']['num_samples']), generator=gen)}


def run(model, batch, draws, **extra):
    """one retraw call under no_grad; injected draws are consumed by a call, so they go in before every one"""
    if draws is not None or extra:
        model.set_random_draws({**(draws or {}), **extra})
    with torch.no_grad():
        return model(batch, retraw=True)


def check_route(tag, plain, fused, state, batch, draws, fp32, f16=False):
    cfg = plain.configs
    m = cfg['model']
    ndc = cfg['data_loader']['ndc']
    s_c, s_f = m['coarse_mlp']['num_samples'], m['fine_mlp']['num_samples']
    count = batch['rays_o'].shape[0]
    training = draws is not None
    # G1
    ops.range_status(clear=True)
    want, got = run(plain, batch, draws), run(fused, batch, draws)
    torch.cuda.synchronize()
    if f16:
        assert ops.range_status() == 0
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(got[k], v), (tag, k, util.linf(got[k], v))
    samples = count * (2 * s_c + s_f)
    assert launches_of(plain, batch) == (2, samples) and launches_of(fused, batch) == (1, samples), tag
    # G2
    near, far = (batch['near_ndc'], batch['far_ndc']) if ndc else (batch['near'], batch['far'])
    z_ref = oracle.coarse_depths(near.cpu(), far.cpu(), s_c, m['lindisp'], draws['t_rand'] if training else None)
    assert util.linf(got['z_vals_coarse'], z_ref) == 0.0, tag
    # G3
    fine_ref = oracle.resample_depths(got['z_vals_coarse'].cpu(), got['weights_coarse'].cpu(), s_f, draws['u'] if training else None)
    differing = int((got['z_vals_fine'].cpu() != fine_ref).sum())
    z = got['z_vals_fine']
    assert torch.all(z[:, 1:] >= z[:, :-1])
    note = f'fused == six-launch on {len(want)} keys, 1 launch vs 2; z_vals_coarse linf 0 [0]; {differing} of {fine_ref.numel()} fine depths differ from the oracle on the device\'s weights [0]'
    if not fp32:
        util.observe(f'routes/{tag}', note)
        assert differing == 0, tag
        return
    # G4
    cpu = {k: v.cpu() for k, v in batch.items()}
    ref = oracle.render(state, cfg, cpu, training=training, retraw=True, rand_per_chunk=[draws] if training else None)
    assert sorted(ref) == sorted(want)
    pinned = run(plain, batch, {'t_rand': draws['t_rand']} if training else None, z_vals_fine=ref['z_vals_fine'])
    assert util.linf(pinned['z_vals_fine'], ref['z_vals_fine']) == 0.0
    for k, v in ref.items():
        level = 'fine' if k.endswith('_fine') else 'coarse'
        out = want if level == 'coarse' else pinned
        bad = per_ray_violation(k, out[k], v.numpy(), ref[f'acc_{level}'].numpy().astype(numpy.float64), ndc)
        if bad is None:
            continue
        assert not bad.any(), (tag, k, int(bad.sum()), util.linf(out[k], v))
    util.observe(f'routes/{tag}', note + f'; vs oracle.render: rays over per_ray_violation\'s bounds 0 [0] on coarse keys and, on the '
                                       f'oracle\'s fine depths, on fine keys; acc_coarse {float(ref["acc_coarse"].mean()):.3f}, '
                                       f'acc_fine {float(ref["acc_fine"].mean()):.3f}')
    assert differing == 0, tag


# (tag, config kind, narrow, overrides, draws) -- the issue's cases a-e
FP32_CASES = [
    ('a/4x128/config2/det', 'config2', True, {}, False),
    ('b/4x128/world128+128/white/det', 'headline_world', True, {'white_bkgd': True}, False),
    ('c/8x256/headline_world/lindisp/det', 'headline_world', False, {'lindisp': True}, False),
    ('d/8x256/config2/draws', 'config2', False, {}, True),
    ('e/4x128/world64+128/lindisp/white/draws', 'headline_world', True, {'lindisp': True, 'white_bkgd': True, 'coarse_samples': 64}, True),
]


@pytest.mark.parametrize('tag,kind,narrow,overrides,with_draws', FP32_CASES, ids=[c[0] for c in FP32_CASES])
def test_fp32_routes_match_each_other_and_the_oracle(tag, kind, narrow, overrides, with_draws):
    plain, fused, state = rc.route_pair(kind, 'fp32', narrow, train=with_draws, raw_noise_std=0.0, **overrides)
    for count in (RAYS, 1) if narrow else (RAYS,):      # the narrow kernels also with a single ray
        batch = rays_of(kind, count)
        check_route(f'{tag}/{count}', plain, fused, state, batch, draws_for(plain, count, 3) if with_draws else None, fp32=True)


@pytest.mark.parametrize('precision', ['bf16', 'f16'])
@pytest.mark.parametrize('kind,overrides', [('headline_world', {'lindisp': True}), ('config2', {})], ids=['f/headline_world/lindisp', 'g/config2'])
def test_16bit_routes_with_draws_match_each_other_and_the_oracles_depths(kind, overrides, precision):
    plain, fused, state = rc.route_pair(kind, precision, False, train=True, raw_noise_std=0.0, **overrides)
    batch = rays_of(kind, RAYS)
    check_route(f'{"f" if overrides else "g"}/{precision}/{kind}/draws', plain, fused, state, batch, draws_for(plain, RAYS, 3),
                fp32=False, f16=precision == 'f16')
