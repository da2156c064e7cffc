"""K4, K5 and K6 on the rays smooth test data never holds (tests/render_cases.py): empty rays, a single opaque sample, a fully
opaque ray, near == far, runs of tied depths, vanishing weights -- stand-alone and through both fused routes.  The reference is
the oracle's own fp32 arithmetic; tests/test_render_cases_host.py pins on the CPU that it is finite and well defined on these
rows and that the facts asserted here as exact bits hold for it.

K6 is gated PER ROW (each row's error against that row's own largest gradient, 1e-5 for d_rgb and 1e-4 for d_sigma): the
per-tensor normalisation of test_composite_backward_matches_autograd would let an opaque neighbour hide a wrong empty ray.  A
row's bound is widened only as far as the oracle alone shows its own gradient to be rounding-limited: the fp32 oracle re-run
with exp one ulp off in either direction gives a band, the bound is max(gate, 2 x band / row max) -- two exp implementations,
each possibly one ulp off -- and a row whose band exceeds 10 % of its own maximum is reported as ungated for that tensor (at
most one row per tensor)."""
import numpy
import pytest
import torch

from oracle import nerf_oracle as oracle
from simplenerf_amd import ops
from tests import render_cases as rc
from tests import util
from tests.test_gpu_kernels import check_resample
from tests.test_gpu_render_routes import check_route, draws_for, rays_of

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SAMPLES = [1, 2, 7, 64, 65, 128, 192, 400, 1024]
GATE_RGB, GATE_SIGMA = 1e-5, 1e-4


def dev(t):
    return None if t is None else t.to(DEV)


# ---------------------------------------------------------------- K5
@pytest.mark.parametrize('s_c,s_f', [(3, 1), (4, 5), (17, 64), (64, 128), (128, 128)])
def test_resample_degenerate_weights_bit_exact(s_c, s_f):
    rng = numpy.random.RandomState(100 * s_c + s_f)
    names, z, w = rc.degenerate_weights(s_c, rng)
    z, w = torch.from_numpy(z), torch.from_numpy(w)
    u = torch.from_numpy(rc.edge_uniforms(len(names), s_f, rng))
    assert bool((u == 0).any(1).all()) and (s_f == 1 or bool((u == numpy.nextafter(numpy.float32(1), numpy.float32(0))).any(1).all()))
    for tag, uu in (('det', None), ('u', u)):
        ref = oracle.resample_depths(z, w, s_f, uu)
        got = ops.resample_depths(dev(z), dev(w), s_f, dev(uu))
        assert got.shape == (len(names), s_c + s_f)
        check_resample(got, ref, z, f'degenerate/c{s_c}_f{s_f}/{tag}')


@pytest.mark.parametrize('s_c,s_f', [(64, 128), (128, 128), (200, 31)])
def test_resample_of_coarse_depths_that_are_not_ascending(s_c, s_f):
    """far within a few ulps of near: the reference's own coarse depths step back and forth (tests/render_cases.py).  Until
    this test resample_wave ranked them by binary search, two elements landed on one slot and the slot left over kept whatever
    the output buffer held (a non-finite fine colour through the model); it now checks the orders it relies on and counts the ranks
    where one does not hold."""
    rng = numpy.random.RandomState(s_c + s_f)
    z = rc.unordered_coarse_depths(s_c)
    assert bool((z[:, 1:] < z[:, :-1]).any(1).all())
    w = torch.from_numpy(rng.gamma(0.4, 0.1, z.shape).astype(numpy.float32))
    u = torch.from_numpy(rc.edge_uniforms(z.shape[0], s_f, rng))
    for tag, uu in (('det', None), ('u', u)):
        ref = oracle.resample_depths(z, w, s_f, uu)
        got = ops.resample_depths(dev(z), dev(w), s_f, dev(uu))
        assert torch.isfinite(got).all()
        check_resample(got, ref, z, f'unordered/c{s_c}_f{s_f}/{tag}')


# ---------------------------------------------------------------- K4
@pytest.mark.parametrize('ndc', [False, True], ids=['world', 'ndc'])
@pytest.mark.parametrize('s', SAMPLES)
def test_composite_degenerate_rows(s, ndc):
    for white in (False, True):
        rng = numpy.random.RandomState(1000 * s + 2 * ndc + white)
        names, t = rc.composite_case(s, ndc, rng)
        ref = oracle.composite(t['sigma'], t['rgb'], t['z'], t['march'], ndc, white, t['rays_o'], t['rays_d'])
        out = ops.composite(dev(t['sigma']), dev(t['rgb']), dev(t['z']), dev(t['march']), ndc, white, dev(t['rays_o']), dev(t['rays_d']))
        out = {k: v.cpu() for k, v in out.items()}
        assert sorted(out) == sorted(ref)
        for k, v in out.items():
            assert torch.isfinite(v).all(), (k, s, ndc, white)
        excluded = rc.depth_excluded_rows(names, ref)
        for i, name in enumerate(names):
            if name == 'empty' or bool((ref['weights'][i] == 0).all()):
                rc.assert_empty_ray_facts(out, i, white, f'K4/{name}/s{s}')
        assert bool((out['alpha'][rc.saturated(t)] == 1).all())
        worst = {}
        for k, v in ref.items():
            if k.startswith('depth'):
                keep = torch.from_numpy(~excluded)
                worst[k] = util.rel_linf(out[k][keep], v[keep])
            else:
                worst[k] = util.rel_linf(out[k], v)
            assert worst[k] < 1e-5, (k, s, ndc, white, worst[k])
        key = max(worst, key=worst.get)
        util.observe(f'composite/degenerate/s{s}/ndc{int(ndc)}/white{int(white)}',
                     f'worst key {key} {worst[key]:.1e} [1e-5] relative; depth-type outputs not compared on '
                     f'{[names[i] for i in numpy.nonzero(excluded)[0]]} (oracle acc <= 1e-2)')


# ---------------------------------------------------------------- K6
def row_bounds(ref_grad, band, gate):
    """per row: (largest entry of the oracle's gradient, bound relative to it or None = ungated)"""
    row_max = ref_grad.double().abs().flatten(1).max(1)[0]
    bounds = []
    for m, b in zip(row_max.tolist(), band.tolist()):
        if m == 0.0:
            bounds.append(0.0)            # the oracle's gradient of this row is exactly 0: so must the kernel's be
        elif b > 0.1 * m:
            bounds.append(None)
        else:
            bounds.append(max(gate, 2.0 * b / m))
    return row_max, bounds


@pytest.mark.parametrize('ndc', [False, True], ids=['world', 'ndc'])
@pytest.mark.parametrize('s', SAMPLES)
def test_composite_backward_degenerate_rows_per_row(s, ndc):
    for white in (False, True):
        rng = numpy.random.RandomState(1000 * s + 2 * ndc + white)
        names, t = rc.composite_case(s, ndc, rng)
        ref = oracle.composite(t['sigma'], t['rgb'], t['z'], t['march'], ndc, white, t['rays_o'], t['rays_d'])
        grads = rc.upstream_gradients(len(names), ndc, rng, ref['acc'])
        want_sigma, want_rgb = rc.composite_gradients(t, ndc, white, grads)
        band_sigma, band_rgb = rc.exp_rounding_band(t, ndc, white, grads)
        d_sigma, d_rgb = ops.composite_backward(dev(t['sigma']), dev(t['rgb']), dev(t['z']), dev(t['march']), ndc, white,
                                                dev(t['rays_o']), dev(t['rays_d']), dev(grads['rgb']), dev(grads['acc']),
                                                dev(grads['depth']), dev(grads['depth_ndc']) if ndc else None)
        d_sigma, d_rgb = d_sigma.cpu(), d_rgb.cpu()
        assert torch.isfinite(d_sigma).all() and torch.isfinite(d_rgb).all()
        assert bool((d_rgb[names.index('empty')] == 0).all())
        failures = []
        for what, got, want, band, gate in (('d_rgb', d_rgb, want_rgb, band_rgb, GATE_RGB), ('d_sigma', d_sigma, want_sigma, band_sigma, GATE_SIGMA)):
            row_max, bounds = row_bounds(want, band, gate)
            err = (got.double() - want.double()).abs().flatten(1).max(1)[0]
            ungated, notes = [], []
            for i, name in enumerate(names):
                m, e, b = float(row_max[i]), float(err[i]), bounds[i]
                if b is None:
                    ungated.append(name)
                    notes.append(f'{name} UNGATED (band {float(band[i]):.1e} of row max {m:.1e}; err {e:.1e})')
                    continue
                rel = e / m if m > 0 else e
                if b > gate:
                    notes.append(f'{name} {rel:.1e} [widened to {b:.1e}: exp band {float(band[i]):.1e} of row max {m:.1e}]')
                if not rel <= b:
                    failures.append((what, name, rel, b, m))
            worst = max((float(err[i]) / float(row_max[i]) for i in range(len(names)) if bounds[i] is not None and float(row_max[i]) > 0), default=0.0)
            util.observe(f'composite_backward/degenerate/s{s}/ndc{int(ndc)}/white{int(white)}/{what}',
                         f'worst row {worst:.1e} [{gate:.0e} of the row\'s own largest entry]' + ('; ' + '; '.join(notes) if notes else ''))
            assert len(ungated) <= 1, (what, ungated)
        assert not failures, failures


# ---------------------------------------------------------------- through the routes
@pytest.mark.parametrize('case', ['d', 'b'])
def test_routes_on_rays_with_near_equal_far(case):
    """Cases (d) (8 x 256, config2, draws) and (b) (4 x 128, world 128 + 128, white) of tests/test_gpu_render_routes.py on rays
    whose near == far -- every coarse depth tied, a flat CDF -- and one ray with far = near (1 + 2^-20): gates G1 to G3 and
    finite outputs (check_route asserts them), through the LDS-tile merge of both fp32 fused kernels."""
    kind, narrow, overrides, with_draws = {'d': ('config2', False, {}, True), 'b': ('headline_world', True, {'white_bkgd': True}, False)}[case]
    plain, fused, state = rc.route_pair(kind, 'fp32', narrow, train=with_draws, raw_noise_std=0.0, **overrides)
    batch = rays_of(kind, 7)
    near_key, far_key = ('near_ndc', 'far_ndc') if kind == 'config2' else ('near', 'far')
    near = torch.full((7, 1), 0.25 if kind == 'config2' else 3.0, device=DEV)
    far = near.clone()
    far[3] = near[3] * (1 + 2.0 ** -20)
    batch[near_key], batch[far_key] = near, far
    check_route(f'near_eq_far/{case}', plain, fused, state, batch, draws_for(plain, 7, 3) if with_draws else None, fp32=False)
