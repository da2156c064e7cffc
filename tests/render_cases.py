"""Shared builders of the render-route and degenerate-ray tests (a plain module, no fixtures): the rays, weights and model
pairs that tests/test_render_cases_host.py pins on the CPU and tests/test_gpu_render_routes.py,
tests/test_gpu_composite_variants.py and tests/test_gpu_degenerate_rays.py feed to the kernels.

The reference for every row is the oracle's own fp32 arithmetic (oracle.composite and autograd through it in float32), not a
float64 evaluation: ``(1 - alpha) + 1e-10`` and ``1 - exp(-x)`` are fp32-specific, and depth = sum(w z) / (acc + 1e-6) is
ill-conditioned at acc ~ 0, so a double-precision run disagrees with the reference itself by up to 100 % on these rows."""
from unittest import mock

import numpy
import torch

from oracle import nerf_oracle as oracle
from simplenerf_amd import synth

ROW_NAMES = ('empty', 'opaque_first', 'opaque_mid', 'opaque_last', 'all_opaque', 'near_eq_far', 'equal_run', 'two_spikes',
             'random')
OPAQUE = 1e4          # sigma of an opaque sample
ACC_GATE = 1e-2       # depth-type quantities are compared where the oracle's acc exceeds this (tests/test_gpu_model.py)


def degenerate_rows(s, ndc, rng):
    """-> (names, z (R,s), sigma (R,s)) float32 arrays, one ray per row: the rays smooth test data never holds.  Depths are
    linspace over [0, 1] (NDC) or [2, 6] (world) unless the row says otherwise; no NaN, no Inf."""
    lo, hi = (0.0, 1.0) if ndc else (2.0, 6.0)
    base = numpy.linspace(lo, hi, s, dtype=numpy.float32)
    z = numpy.tile(base, (len(ROW_NAMES), 1))
    sigma = numpy.zeros((len(ROW_NAMES), s), dtype=numpy.float32)
    row = {name: i for i, name in enumerate(ROW_NAMES)}
    sigma[row['opaque_first'], 0] = OPAQUE
    sigma[row['opaque_mid'], s // 2] = OPAQUE
    sigma[row['opaque_last'], s - 1] = OPAQUE
    sigma[row['all_opaque']] = OPAQUE
    z[row['near_eq_far']] = numpy.float32(0.5 * (lo + hi))
    sigma[row['near_eq_far']] = rng.gamma(0.5, 8.0, s)
    k = max(0, min(s // 2 - 1, s - 3))
    z[row['equal_run'], k:k + 3] = z[row['equal_run'], k]
    sigma[row['equal_run']] = rng.gamma(0.5, 8.0, s)
    k = min(s // 3, max(0, s - 2))
    sigma[row['two_spikes'], k] = 35.0
    if k + 1 < s:
        sigma[row['two_spikes'], k + 1] = 15.0
    z[row['random']] = numpy.sort(rng.uniform(lo, hi, s).astype(numpy.float32))
    sigma[row['random']] = rng.gamma(0.5, 8.0, s)
    sigma[row['random']][rng.uniform(size=s) < 0.3] = 0
    return list(ROW_NAMES), z, sigma


DEPTH_FAMILIES = ('sorted_random', 'linspace', 'all_equal', 'equal_run')
WEIGHT_FAMILIES = ('all_zero', 'one_hot', 'two_spikes', 'mostly_zero', 'vanishing', 'random')


def degenerate_weights(s_c, rng):
    """-> (names, z (R,s_c), weights (R,s_c)) for K5 alone: every depth family x every weight family, depths in [0, 1]."""
    names, zs, ws = [], [], []
    for df in DEPTH_FAMILIES:
        for wf in WEIGHT_FAMILIES:
            if df == 'sorted_random':
                z = numpy.sort(rng.uniform(0, 1, s_c))
            elif df == 'linspace':
                z = numpy.linspace(0, 1, s_c)
            elif df == 'all_equal':
                z = numpy.full(s_c, 0.375)
            else:
                z = numpy.linspace(0, 1, s_c)
                k = max(0, min(s_c // 2 - 1, s_c - 3))
                z[k:k + 3] = z[k]
            w = numpy.zeros(s_c)
            spot = min(s_c // 3 + 1, s_c - 1)
            if wf == 'one_hot':
                w[spot] = 1.0
            elif wf == 'two_spikes':
                w[spot] = 0.6
                w[max(spot - 1, 0)] = 0.4
            elif wf == 'mostly_zero':
                w = rng.gamma(0.4, 0.1, s_c) * (rng.uniform(size=s_c) >= 0.7)
            elif wf == 'vanishing':
                w = rng.gamma(0.4, 0.1, s_c) * 1e-30
            elif wf == 'random':
                w = rng.gamma(0.4, 0.1, s_c)
            names.append(f'{df}/{wf}')
            zs.append(z.astype(numpy.float32))
            ws.append(w.astype(numpy.float32))
    return names, numpy.stack(zs), numpy.stack(ws)


def edge_uniforms(n, s_f, rng):
    """u (n, s_f) in [0, 1) whose rows hold an exact 0.0 and nextafter(1, 0) (as many of the two as s_f has room for)"""
    u = rng.uniform(0, 1, (n, s_f)).astype(numpy.float32)
    u[:, 0] = 0.0
    if s_f > 1:
        u[:, s_f - 1 - (s_f > 2)] = numpy.nextafter(numpy.float32(1), numpy.float32(0))
    return u


def inverse_cdf_samples(z_coarse, weights_coarse, num_fine, u=None):
    """The samples of oracle.resample_depths before its cat + sort (the same tensor ops in the same order; the host test
    checks that sorting [z_coarse | these] reproduces the oracle bit for bit)."""
    bins = .5 * (z_coarse[..., 1:] + z_coarse[..., :-1])
    w = weights_coarse[..., 1:-1] + 1e-5
    pdf = w / torch.sum(w, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    if u is None:
        u = torch.linspace(0., 1., steps=num_fine).expand(list(cdf.shape[:-1]) + [num_fine])
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(inds - 1, min=0)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1)
    cdf_b, cdf_a = torch.gather(cdf, -1, below), torch.gather(cdf, -1, above)
    bin_b, bin_a = torch.gather(bins, -1, below), torch.gather(bins, -1, above)
    denom = cdf_a - cdf_b
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_b) / denom
    return bin_b + t * (bin_a - bin_b)


def rank_merge(z_coarse, samples, drawn):
    """numpy restatement of resample_wave's merge (csrc/resample_device.h): every element of [coarse | samples] is scattered
    to its rank.  With ascending coarse depths: coarse j to j + #{samples < z_j}, sample k to #{coarse <= s_k} + its rank among
    the samples -- k itself when the samples come from the deterministic linspace (``drawn`` False) and are ascending, else
    #{s_q < s_k or (s_q == s_k and q < k)}.  When an order it would rely on does not hold, every element's rank is counted in
    the concatenation under (value, position).  -> (merged, every slot written exactly once)"""
    s_c, s_f = len(z_coarse), len(samples)
    ascending = bool((z_coarse[:-1] <= z_coarse[1:]).all()) and (drawn or bool((samples[:-1] <= samples[1:]).all()))
    out = numpy.full(s_c + s_f, numpy.nan, dtype=numpy.float32)
    written = numpy.zeros(s_c + s_f, dtype=numpy.int64)
    if not ascending:
        both = numpy.concatenate([z_coarse, samples])
        for i, v in enumerate(both):
            rank = int(((both < v) | ((both == v) & (numpy.arange(s_c + s_f) < i))).sum())
            out[rank] = v
            written[rank] += 1
        return out, bool((written == 1).all())
    for j, v in enumerate(z_coarse):
        below = int((samples < v).sum()) if drawn else int(numpy.searchsorted(samples, v, side='left'))
        out[j + below] = v
        written[j + below] += 1
    for k, v in enumerate(samples):
        lo = int(numpy.searchsorted(z_coarse, v, side='right'))
        among = int(((samples < v) | ((samples == v) & (numpy.arange(s_f) < k))).sum()) if drawn else k
        out[lo + among] = v
        written[lo + among] += 1
    return out, bool((written == 1).all())


def unordered_coarse_depths(s_c, n=6):
    """The reference's own coarse depths of rays whose far is within a few ulps of near: near (1 - t) + far t rounds three
    times, so over such a range the depths step back and forth (NOT ascending) -- world rays, near in [2, 4), far = near
    (1 + 2^-20 .. 2^-18).  -> z (n, s_c) float32 tensor"""
    near = torch.linspace(2.5, 3.75, n)[:, None]
    far = near * (1 + 2.0 ** -torch.tensor([20., 19., 18.]).repeat(n)[:n, None])
    return oracle.coarse_depths(near, far, s_c)


# ---------------------------------------------------------------------------------------------- compositing cases
def composite_case(s, ndc, rng):
    """Rays around degenerate_rows: (names, tensors) with z, sigma, rgb, march directions and, for NDC, the world rays of the
    committed compositing fixture (their NDC directions belong to them)."""
    from tests import util
    names, z, sigma = degenerate_rows(s, ndc, rng)
    n = len(names)
    t = {'z': torch.from_numpy(z), 'sigma': torch.from_numpy(sigma),
         'rgb': torch.from_numpy(rng.uniform(0, 1, (n, s, 3)).astype(numpy.float32)), 'rays_o': None, 'rays_d': None}
    if ndc:
        g = util.load('composite.npz')
        t['rays_o'], t['rays_d'] = torch.from_numpy(g['ndc_s64_rays_o'][:n]), torch.from_numpy(g['ndc_s64_rays_d'][:n])
        t['march'] = torch.from_numpy(g['ndc_s64_rays_d_ndc'][:n])
    else:
        t['march'] = torch.from_numpy(rng.standard_normal((n, 3)).astype(numpy.float32))
    return names, t


def _exp_off_by_one_ulp(direction):
    """torch.exp whose non-zero results of non-zero arguments are moved one ulp towards +-inf, with exp's own backward (grad
    times the returned value)"""
    real_exp = torch.exp

    class Exp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            e = real_exp(x)
            moved = torch.nextafter(e, torch.full_like(e, direction * float('inf')))
            e = torch.where((x != 0) & (e != 0), moved, e)
            ctx.save_for_backward(e)
            return e

        @staticmethod
        def backward(ctx, grad):
            return grad * ctx.saved_tensors[0]

    return Exp.apply


def composite_gradients(t, ndc, white, upstream, exp=None):
    """fp32 autograd through oracle.composite -> (d_sigma, d_rgb).  ``exp``: a replacement for torch.exp inside the oracle."""
    sg, cg = t['sigma'].clone().requires_grad_(True), t['rgb'].clone().requires_grad_(True)
    if exp is None:
        out = oracle.composite(sg, cg, t['z'], t['march'], ndc, white, t['rays_o'], t['rays_d'])
    else:
        with mock.patch.object(torch, 'exp', exp):
            out = oracle.composite(sg, cg, t['z'], t['march'], ndc, white, t['rays_o'], t['rays_d'])
    sum((out[k] * upstream[k]).sum() for k in upstream if k in out).backward()
    return sg.grad, cg.grad


def exp_rounding_band(t, ndc, white, upstream):
    """Per row, how far the oracle's own gradients move when its exp is one ulp off in either direction -- measured from the
    oracle alone.  -> (band_sigma (R,), band_rgb (R,)) absolute."""
    d_sigma, d_rgb = composite_gradients(t, ndc, white, upstream)
    band_s = torch.zeros(d_sigma.shape[0], dtype=torch.float64)
    band_c = torch.zeros(d_sigma.shape[0], dtype=torch.float64)
    for direction in (-1.0, 1.0):
        ps, pc = composite_gradients(t, ndc, white, upstream, _exp_off_by_one_ulp(direction))
        band_s = torch.maximum(band_s, (ps.double() - d_sigma.double()).abs().flatten(1).max(1)[0])
        band_c = torch.maximum(band_c, (pc.double() - d_rgb.double()).abs().flatten(1).max(1)[0])
    return band_s, band_c


# ---------------------------------------------------------------------------------------------- model pairs
def one_launch_resample(s_c, s_f):
    """csrc/render.hip's condition for compositing + resampling the main coarse level in ONE kernel (composite_resample):
    four rays' tiles and scratch inside 64 KiB of LDS"""
    return s_c >= 3 and 4 * 4 * (2 * s_c + s_f + 2 * (s_c - 1)) <= 64 * 1024


def route_configs(kind, precision='fp32', narrow=False, fused=False, coarse_samples=None, fine_samples=None, **overrides):
    cfg = synth.with_overrides(synth.make_configs(kind), hip_precision=precision, hip_fused_render=fused, **overrides)
    for level, samples in (('coarse_mlp', coarse_samples), ('fine_mlp', fine_samples)):
        if samples:
            cfg['model'][level]['num_samples'] = samples
        if narrow:      # 4 x 128, views width 64 (as pair_narrow of tests/test_gpu_fused16.py)
            cfg['model'][level].update(synth.mlp_config(cfg['model'][level]['num_samples'], depth=4, width=128, views_width=64))
    return cfg


def route_pair(kind, precision='fp32', narrow=False, train=False, device='cuda:0', fused=(False, True), **overrides):
    """(six-launch model, fused model) with the same synthetic weights -- synth_state_dict(shapes, 11, 150.0, 4.0), the field of
    _oracle_vs_model (tests/test_gpu_model.py) -- and that state dict on the CPU for the oracle"""
    from simplenerf_amd.models.ModelFactory import get_model
    models, state = [], None
    for flag in fused:
        model = get_model(route_configs(kind, precision, narrow, flag, **overrides), None)
        if state is None:
            shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
            state = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 11, 150.0, 4.0).items()}
        model.load_state_dict(state)
        models.append(model.to(device).train(train))
    return models + [state]


# ---------------------------------------------------------------------------------------------- facts both sides assert
def upstream_gradients(n, ndc, rng, acc):
    """Per-ray upstream gradients of K6 (rgb, acc, depth[, depth_ndc]); the depth ones zeroed on rays whose oracle acc is
    <= ACC_GATE, where depth = sum(w z) / (acc + 1e-6) -- and with it its gradient -- is ill-conditioned"""
    grads = {k: torch.from_numpy(rng.standard_normal(shape).astype(numpy.float32))
             for k, shape in (('rgb', (n, 3)), ('acc', (n,)), ('depth', (n,)), ('depth_ndc', (n,)))}
    if not ndc:
        del grads['depth_ndc']
    low = torch.as_tensor(acc) <= ACC_GATE
    for k in ('depth', 'depth_ndc'):
        if k in grads:
            grads[k][low] = 0
    return grads


def depth_excluded_rows(names, ref):
    """bool (R,): rows whose depth-type outputs are not compared (oracle acc <= ACC_GATE).  Only 'empty', 'near_eq_far' and
    'equal_run' may be among them -- and a row that IS an empty ray: every oracle weight exactly 0 (in NDC the last depth is
    1 = the far cap, so the last sample's delta is 0 and a ray that is opaque only there composites to nothing); such a row
    is held to the empty row's exact facts instead."""
    low = (ref['acc'] <= ACC_GATE).numpy()
    for i in numpy.nonzero(low)[0]:
        assert names[i] in ('empty', 'near_eq_far', 'equal_run') or bool((ref['weights'][i] == 0).all()), (names[i], float(ref['acc'][i]))
    return low


def assert_empty_ray_facts(out, i, white, who):
    """Exact bits of a ray without density: alpha, weights, acc, depths and their variances 0, visibility 1 (1 + 1e-10 rounds
    to 1), colour 0 -- or exactly 1 on a white background"""
    for k in ('alpha', 'weights', 'acc', 'depth', 'depth_var', 'depth_ndc', 'depth_var_ndc'):
        if k in out:
            assert bool((out[k][i] == 0).all()), (who, k, out[k][i])
    assert bool((out['visibility'][i] == 1).all()), (who, 'visibility')
    assert bool((out['rgb'][i] == (1.0 if white else 0.0)).all()), (who, 'rgb', out['rgb'][i])


def saturated(t):
    """bool (R,S): samples with sigma * delta >= 104 in the oracle's fp32 delta: exp(-104) is below the smallest fp32
    denormal, so alpha is exactly 1 there"""
    ndc = t['rays_o'] is not None
    far_cap = torch.tensor([1. if ndc else 1e10])
    z1 = torch.cat([t['z'], far_cap.expand(t['z'][..., :1].shape)], -1)
    delta = (z1[..., 1:] - z1[..., :-1]) * torch.norm(t['march'][..., None, :], dim=-1)
    return t['sigma'] * delta >= 104
