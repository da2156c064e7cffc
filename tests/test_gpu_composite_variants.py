"""The compositing instantiations no other test runs.  composite_kernel<C> / composite_backward_kernel<C> are compiled for
C = ceil(S / 64) in {1, 2, 3, 4, 6, 8, 16}: stand-alone the backward ran at C in {1, 3, 4} only (C = 6, 8, 16 nowhere), the
forward never at C = 8, and the one-launch compositing + resampling form (composite_resample) only at the shipped 64 and 128
coarse samples (C = 1, 2).  Same recipes, references and gates as their neighbours in tests/test_gpu_grads.py and
tests/test_gpu_kernels.py."""
import numpy
import pytest
import torch

from oracle import nerf_oracle as oracle
from simplenerf_amd import ops, synth
from tests import render_cases as rc
from tests import util
from tests.test_gpu_grads import rel_to_max
from tests.test_gpu_model import per_ray_violation

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

BACKWARD_SAMPLES = [65, 128, 257, 384, 385, 512, 513, 1024]          # C = 2, 2, 6, 6, 8, 8, 16, 16


def lane_block(s):
    """the instantiation composite.hip selects for s samples per ray: C samples per lane, C >= ceil(s / 64)"""
    return next(c for c in (1, 2, 3, 4, 6, 8, 16) if 64 * c >= s)
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize('s', BACKWARD_SAMPLES)
def test_composite_backward_matches_autograd_at_every_lane_block_size(s):
    """the recipe of test_composite_backward_matches_autograd (its opaque sample and its two empty rows included) against fp32
    autograd through oracle.composite, (ndc, white) rotating over the sample counts"""
    ndc, white = VARIANTS[BACKWARD_SAMPLES.index(s) % 4]
    rng = numpy.random.RandomState(s + 17 * ndc)
    n = 9
    if ndc:
        g = util.load('composite.npz')
        rays_o, rays_d = torch.from_numpy(g['ndc_s64_rays_o'][:n]), torch.from_numpy(g['ndc_s64_rays_d'][:n])
        march = torch.from_numpy(g['ndc_s64_rays_d_ndc'][:n])
        z = torch.from_numpy(numpy.sort(rng.uniform(0, 1, (n, s)).astype(numpy.float32), axis=1))
        z[: n // 2] = torch.linspace(0, 1, s)
    else:
        rays_o = rays_d = None
        march = torch.from_numpy(rng.standard_normal((n, 3)).astype(numpy.float32))
        z = torch.from_numpy(numpy.sort(rng.uniform(2, 6, (n, s)).astype(numpy.float32), axis=1))
    sigma = torch.from_numpy(rng.gamma(0.5, 8.0, (n, s)).astype(numpy.float32))
    sigma[rng.uniform(size=sigma.shape) < 0.3] = 0
    sigma[:2] = 0
    sigma[2:4, 5 % s] = 1e4  # an opaque sample: 1 - alpha + 1e-10 = 1e-10
    rgb = torch.from_numpy(rng.uniform(0, 1, (n, s, 3)).astype(numpy.float32))
    grads = {k: torch.from_numpy(rng.standard_normal(shape).astype(numpy.float32))
             for k, shape in (('rgb', (n, 3)), ('acc', (n,)), ('depth', (n,)), ('depth_ndc', (n,)))}
    sg, cg = sigma.clone().requires_grad_(True), rgb.clone().requires_grad_(True)
    out = oracle.composite(sg, cg, z, march, ndc, white, rays_o, rays_d)
    loss = sum((out[k] * grads[k]).sum() for k in grads if k in out)
    loss.backward()
    d = lambda t: None if t is None else t.to(DEV)
    d_sigma, d_rgb = ops.composite_backward(d(sigma), d(rgb), d(z), d(march), ndc, white, d(rays_o), d(rays_d),
                                            d(grads['rgb']), d(grads['acc']), d(grads['depth']),
                                            d(grads['depth_ndc']) if ndc else None)
    assert torch.isfinite(d_sigma).all() and torch.isfinite(d_rgb).all()
    e_rgb, e_sigma = rel_to_max(d_rgb, cg.grad), rel_to_max(d_sigma, sg.grad)
    util.observe(f'composite_backward/s{s}/ndc{int(ndc)}/white{int(white)}',
                 f'C = {lane_block(s)}: d_rgb {e_rgb:.1e} [1e-5], d_sigma {e_sigma:.1e} [1e-4] of the largest entry')
    assert e_rgb < 1e-5
    assert e_sigma < 1e-4


@pytest.mark.parametrize('s', [385, 400, 512])
def test_composite_forward_at_eight_samples_per_lane(s):
    """test_composite_ragged_sample_counts' check at the sample counts that select composite_kernel<8>"""
    rng = numpy.random.RandomState(s)
    n = 9
    z = torch.from_numpy(numpy.sort(rng.uniform(2, 6, (n, s)).astype(numpy.float32), axis=1))
    sigma = torch.from_numpy(rng.gamma(0.5, 4.0, (n, s)).astype(numpy.float32))
    rgb = torch.from_numpy(rng.uniform(0, 1, (n, s, 3)).astype(numpy.float32))
    d = torch.from_numpy(rng.standard_normal((n, 3)).astype(numpy.float32))
    ref = oracle.composite(sigma, rgb, z, d, False)
    out = ops.composite(sigma.to(DEV), rgb.to(DEV), z.to(DEV), d.to(DEV), False)
    worst = 0.0
    for k, v in ref.items():
        err = util.rel_linf(out[k], v)
        worst = max(worst, err)
        assert err < 1e-5, k
    util.observe(f'composite/s{s}', f'C = 8: worst key {worst:.1e} [1e-5] relative')


@pytest.mark.parametrize('s_c,s_f', [(192, 64), (256, 128), (300, 64), (450, 64), (1000, 24)])
def test_composite_and_resample_in_one_launch_at_every_lane_block_size(s_c, s_f):
    """K4 + K5 as one kernel (composite_resample, RESAMPLE = true) at C = 3, 4, 6, 8 and 16, through a six-launch 4 x 128 model
    on five world rays: coarse depths and merged fine depths bit-equal to the oracle's (the latter on the device's own
    weights), coarse-level outputs inside per_ray_violation's bounds on every ray."""
    eligible = rc.one_launch_resample(s_c, s_f)
    util.observe(f'composite_resample/{s_c}+{s_f}', f'C = {lane_block(s_c)}; render.hip takes the one-launch form: {eligible}')
    assert eligible, 'this pair would run K4 and K5 as two kernels: move it to the nearest pair of the same C that fits 64 KiB'
    (plain, state) = rc.route_pair('headline_world', 'fp32', True, fused=(False,), coarse_samples=s_c, fine_samples=s_f)
    cfg = plain.configs
    rays = synth.random_world_rays(5, seed=s_c)
    batch = {k: torch.from_numpy(v).to(DEV) for k, v in rays.items()}
    with torch.no_grad():
        out = plain(batch, retraw=True)
    assert all(torch.isfinite(v).all() for v in out.values())
    ref = oracle.render(state, cfg, {k: torch.from_numpy(v) for k, v in rays.items()}, training=False, retraw=True)
    assert util.linf(out['z_vals_coarse'], ref['z_vals_coarse']) == 0.0
    fine_ref = oracle.resample_depths(out['z_vals_coarse'].cpu(), out['weights_coarse'].cpu(), s_f)
    differing = int((out['z_vals_fine'].cpu() != fine_ref).sum())
    acc = ref['acc_coarse'].numpy().astype(numpy.float64)
    assert float(acc.mean()) > 0.05, 'the coarse pass must not be empty'
    for k, v in ref.items():
        if not k.endswith('_coarse'):
            continue
        bad = per_ray_violation(k, out[k], v.numpy(), acc, False)
        assert bad is None or not bad.any(), (k, util.linf(out[k], v))
    util.observe(f'composite_resample/{s_c}+{s_f}', f'{differing} of {fine_ref.numel()} merged depths differ from the oracle on the '
                                                    f'device\'s weights [0]; coarse keys: 0 rays over the bounds [0]; acc_coarse {acc.mean():.3f}')
    assert differing == 0
