"""The conditions under which the GPU gates of tests/test_gpu_degenerate_rays.py and tests/test_gpu_render_routes.py are fair,
pinned on the CPU (no GPU needed): on every degenerate row (tests/render_cases.py) the fp32 oracle and fp32 autograd through it
are finite, the facts the GPU tests assert as exact bits hold for the oracle itself, and resample_wave's merge by rank -- here
restated in numpy and fed with the oracle's own fp32 inverse-CDF samples -- is a sort, ties and flat CDFs included, so
bit-exactness of the resampled depths is a fair demand on those rows."""
import numpy
import pytest
import torch

from oracle import nerf_oracle as oracle
from tests import render_cases as rc

SAMPLES = [1, 2, 7, 64, 65, 128, 192, 400, 1024]


@pytest.mark.parametrize('ndc', [False, True], ids=['world', 'ndc'])
@pytest.mark.parametrize('s', SAMPLES)
def test_oracle_is_finite_and_exact_on_degenerate_rows(s, ndc):
    for white in (False, True):
        rng = numpy.random.RandomState(1000 * s + 2 * ndc + white)
        names, t = rc.composite_case(s, ndc, rng)
        ref = oracle.composite(t['sigma'], t['rgb'], t['z'], t['march'], ndc, white, t['rays_o'], t['rays_d'])
        for k, v in ref.items():
            assert torch.isfinite(v).all(), (k, s, ndc, white)
        low = rc.depth_excluded_rows(names, ref)
        for i, name in enumerate(names):
            if name == 'empty' or bool((ref['weights'][i] == 0).all()):
                rc.assert_empty_ray_facts(ref, i, white, f'oracle/{name}')
        assert low[names.index('empty')]
        sat = rc.saturated(t)
        assert bool((ref['alpha'][sat] == 1).all())
        grads = rc.upstream_gradients(len(names), ndc, rng, ref['acc'])
        d_sigma, d_rgb = rc.composite_gradients(t, ndc, white, grads)
        assert torch.isfinite(d_sigma).all() and torch.isfinite(d_rgb).all(), (s, ndc, white)
        assert bool((d_rgb[names.index('empty')] == 0).all())
        band_s, band_c = rc.exp_rounding_band(t, ndc, white, grads)
        assert torch.isfinite(band_s).all() and torch.isfinite(band_c).all()


@pytest.mark.parametrize('s_c', [3, 4, 17, 64, 128])
def test_merge_by_rank_is_a_sort_on_degenerate_weights(s_c):
    rng = numpy.random.RandomState(s_c)
    names, z, w = rc.degenerate_weights(s_c, rng)
    zt, wt = torch.from_numpy(z), torch.from_numpy(w)
    for s_f in (1, 5, 64, 128):
        for u in (None, torch.from_numpy(rc.edge_uniforms(len(names), s_f, rng))):
            samples = rc.inverse_cdf_samples(zt, wt, s_f, u)
            assert torch.isfinite(samples).all()
            ref = oracle.resample_depths(zt, wt, s_f, u)
            assert torch.equal(torch.sort(torch.cat([zt, samples], -1), -1)[0], ref)      # the restated samples are the oracle's
            if u is None:     # the inverse CDF of ascending u is ascending here: the kernel ranks these rows by binary search
                assert bool((samples[:, 1:] >= samples[:, :-1]).all()), s_f
            for i, name in enumerate(names):
                merged, once = rc.rank_merge(z[i], samples[i].numpy(), drawn=u is not None)
                assert once, (name, s_f)
                assert numpy.array_equal(merged, ref[i].numpy()), (name, s_f, u is None)


@pytest.mark.parametrize('s_c,s_f', [(64, 128), (128, 128), (200, 31)])
def test_merge_by_rank_is_a_sort_when_the_references_coarse_depths_are_not_ascending(s_c, s_f):
    """far within a few ulps of near: the reference's coarse depths (and with them the bin mid-points and the deterministic
    samples) are not ascending; ranks found by binary search would then collide, counted ranks do not."""
    rng = numpy.random.RandomState(s_c + s_f)
    z = rc.unordered_coarse_depths(s_c)
    assert bool((z[:, 1:] < z[:, :-1]).any(1).all()), 'every row must step backwards somewhere'
    w = torch.from_numpy(rng.gamma(0.4, 0.1, z.shape).astype(numpy.float32))
    for u in (None, torch.from_numpy(rc.edge_uniforms(z.shape[0], s_f, rng))):
        samples = rc.inverse_cdf_samples(z, w, s_f, u)
        ref = oracle.resample_depths(z, w, s_f, u)
        assert torch.isfinite(ref).all()
        for i in range(z.shape[0]):
            merged, once = rc.rank_merge(z[i].numpy(), samples[i].numpy(), drawn=u is not None)
            assert once and numpy.array_equal(merged, ref[i].numpy()), (i, u is None)
