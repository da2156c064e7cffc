"""The field's gradient and the normals it gives, restated for the tests: ``normals`` is simplenerf_amd/csrc/simplenerf_gradient.h's
rule for snerf_field_normals in plain Python floats (IEEE doubles, one operation per step, in the header's order, nothing fused),
point by point; the gradient ORACLE is the autograd of ``oracle.nerf_oracle.mlp_forward``'s sigma with respect to its points, in
float64, and once more in float32 -- the distance between those two is the error an fp32 evaluation of this gradient has anyway, and
four times it (the margin of tests/test_field_host.py) is the bound the device is held to.

The gradient of a ReLU network jumps where a hidden pre-activation crosses 0, so a point is COMPARED only where, in the float64
forward, every hidden (trunk) pre-activation is farther from 0 than 1e-5 (the fp32 forward tests' tolerance) times the largest
magnitude of that layer's pre-activations over the case's points.  The cases below (weights' seed, density head's gain and shift,
the box of the points) were chosen on the CPU with the oracle alone so that at most a quarter of a case's points is left out and
at least half of the compared ones have sigma > 0; tests/test_field_gradient_host.py asserts both and records the shares."""
import functools
import math

import numpy
import torch

from oracle import nerf_oracle as oracle

from . import field_reference

_divide = field_reference._divide
HIDDEN_MARGIN = 1e-5          # tests/test_gpu_kernels.py holds the fp32 forward to the oracle at 1e-5
BOUND_FACTOR = 4.0
POINT_COUNTS = (1, 31, 32, 33, 129, 300)      # the 32-sample tile's edge, the 128-sample workgroup's edge, three workgroups


# ---------------------------------------------------------------------------------------------------------------- the normals
def normals(points, grad, ndc=None):
    """snerf_field_normals -> float32 (count, 3)."""
    points = numpy.asarray(points, dtype=numpy.float32)
    grad = numpy.asarray(grad, dtype=numpy.float32)
    out = numpy.zeros((len(points), 3), dtype=numpy.float32)
    for at in range(len(points)):
        P = [float(v) for v in points[at]]
        g = [float(v) for v in grad[at]]
        G, in_front = list(g), True
        with numpy.errstate(all='ignore'):
            if ndc is not None:
                cx, cy, near = (float(v) for v in ndc)
                in_front = bool(P[2] <= -near)
                G[0] = _divide(cx, P[2]) * g[0]
                G[1] = _divide(cy, P[2]) * g[1]
                G[2] = -_divide(((cx * P[0]) * g[0] + (cy * P[1]) * g[1]) + (2.0 * near) * g[2], P[2] * P[2])
            m = float(numpy.sqrt(numpy.float64((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])))
            if in_front and m > 0.0 and m < math.inf:
                out[at] = [numpy.float32(_divide(-G[a], m)) for a in range(3)]
    return out


def ndc_map(P, ndc):
    """THE INPUT MAP's Q of a point in front (tests/field_reference.py input_point)."""
    return field_reference.input_point([float(v) for v in P], ndc)[0]


def pull_back(P, g, ndc):
    """J^T g of the restated rule, unnormalised (three floats)."""
    cx, cy, near = (float(v) for v in ndc)
    return [_divide(cx, P[2]) * g[0], _divide(cy, P[2]) * g[1],
            -_divide(((cx * P[0]) * g[0] + (cy * P[1]) * g[1]) + (2.0 * near) * g[2], P[2] * P[2])]


# the analytic ball of tests/field_reference.py: sigma = 40 max(0, 1 - |p| / 1.2) and its gradient -(40 / 1.2) p / |p| inside
def ball_gradient(points):
    points = numpy.asarray(points, dtype=numpy.float64)
    radius = numpy.linalg.norm(points, axis=1, keepdims=True)
    inside = (radius < 1.2) & (radius > 0)
    return numpy.where(inside, -(40.0 / 1.2) * points / numpy.where(radius > 0, radius, 1.0), 0.0).astype(numpy.float32)


# ---------------------------------------------------------------------------------------------------------------- the oracle's cases
# name: (MLP overrides of synth.mlp_config, weights' seed, density gain, density shift, half-width of the points' box, points' seed)
CASES = {
    'w256_views': (dict(depth=8, width=256, views_width=128), 31, 50.0, 2.75, 1.0, 5),
    'w256_plain': (dict(depth=8, width=256, use_view_dirs=False, view_dependent_rgb=False), 32, 50.0, 1.0, 1.0, 6),
    'w128_views': (dict(depth=8, width=128, views_width=64), 33, 50.0, 0.5, 1.0, 7),
    'w128_plain': (dict(depth=8, width=128, use_view_dirs=False, view_dependent_rgb=False), 34, 50.0, -2.0, 1.0, 8),
    'w256_ptsaug': (dict(depth=8, width=256, views_width=128, sigma_pe_degree=3), 35, 50.0, 1.25, 1.0, 9),
    'w128_d4': (dict(depth=4, width=128, views_width=64), 36, 50.0, 1.0, 1.0, 10),       # no skip layer: W_0 alone
}
# What the oracle gives for them (asserted by tests/test_field_gradient_host.py): (share of points left out, share of the compared
# points with sigma > 0, the float32 oracle's error relative to max |grad|); every case's first point is compared and has sigma > 0.
RECORDED = {
    'w256_views': (0.083, 0.836, 4.587e-07),
    'w256_plain': (0.060, 0.890, 4.291e-07),
    'w128_views': (0.030, 0.711, 5.260e-07),
    'w128_plain': (0.040, 0.688, 3.633e-07),
    'w256_ptsaug': (0.033, 0.986, 3.647e-07),
    'w128_d4': (0.007, 0.876, 3.509e-07),
}
PREFIX = 'coarse_model.'


def case_configs(name, precision='fp32'):
    """The experiment configs of a case: config1 (world-space rays, a coarse MLP only) with the case's MLP."""
    from simplenerf_amd import synth
    cfg = synth.with_overrides(synth.make_configs('config1'), hip_precision=precision)
    cfg['model']['coarse_mlp'] = synth.mlp_config(64, **CASES[name][0])
    return cfg


@functools.lru_cache(maxsize=None)
def case_state(name):
    """{key: float32 tensor}: the seeded weights of a case's model, under the model's own names."""
    from simplenerf_amd import synth
    from . import util
    _, seed, gain, shift, _, _ = CASES[name]
    shapes = util.model_param_shapes(case_configs(name))
    return {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed, gain, shift).items()}


def _sigma_and_gradient(state, mlp_cfg, points, dtype):
    params = {k: v.to(dtype) for k, v in state.items()}
    pts = torch.from_numpy(numpy.array(points)).to(dtype).requires_grad_(True)
    dirs = None
    if mlp_cfg['use_view_dirs']:
        dirs = torch.tensor([0.0, 0.0, -1.0], dtype=dtype).expand(len(points), 3)
    sigma = oracle.mlp_forward(params, PREFIX, mlp_cfg, pts, dirs)['sigma'][:, 0]
    sigma.sum().backward()            # (the points are independent: row i of the gradient is d sigma_i / d x_i)
    return sigma.detach().numpy(), pts.grad.detach().numpy()


def hidden_margins(state, mlp_cfg, points):
    """-> (count,) float64: per point the smallest, over the trunk's layers, of min |pre-activation| / (the layer's largest
    |pre-activation| over all points), in the float64 restatement of the trunk of oracle.nerf_oracle.mlp_forward."""
    params = {k: v.double() for k, v in state.items()}
    lay = oracle.mlp_layout(params, PREFIX)
    enc = oracle.pos_encode(torch.from_numpy(numpy.array(points)).double(), mlp_cfg['points_positional_encoding_degree'])
    trunk_in = enc[:, :lay['pts_in']]
    h = trunk_in
    worst = torch.full((len(points),), math.inf, dtype=torch.float64)
    for i in range(lay['depth']):
        z = torch.nn.functional.linear(h, params[f'{PREFIX}pts_linears.{i}.weight'], params[f'{PREFIX}pts_linears.{i}.bias'])
        worst = torch.minimum(worst, z.abs().min(dim=1)[0] / z.abs().max())
        h = torch.relu(z)
        if i == oracle.SKIP_AFTER_LAYER:
            h = torch.cat([trunk_in, h], -1)
    return worst.numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything the tests need of a case, computed once on the CPU; arrays are read-only.
    points float32 (300, 3); sigma, grad: the float64 oracle; compared: bool (300,); measured: the float32 oracle's largest
    |grad32 - grad| over the compared points relative to max |grad| over them; bound = 4 x measured; left_out, positive: shares."""
    _, _, _, _, half_width, points_seed = CASES[name]
    mlp_cfg = case_configs(name)['model']['coarse_mlp']
    state = case_state(name)
    rng = numpy.random.RandomState(points_seed)
    points = rng.uniform(-half_width, half_width, (POINT_COUNTS[-1], 3)).astype(numpy.float32)
    sigma, grad = _sigma_and_gradient(state, mlp_cfg, points, torch.float64)
    sigma32, grad32 = _sigma_and_gradient(state, mlp_cfg, points, torch.float32)
    compared = hidden_margins(state, mlp_cfg, points) > HIDDEN_MARGIN
    scale = float(numpy.abs(grad[compared]).max())
    measured = float(numpy.abs(grad32[compared].astype(numpy.float64) - grad[compared]).max()) / scale
    out = {'points': points, 'sigma': sigma, 'grad': grad, 'sigma32': sigma32, 'grad32': grad32, 'compared': compared, 'scale': scale,
           'measured': measured, 'bound': BOUND_FACTOR * measured, 'left_out': float(1.0 - compared.mean()),
           'positive': float((sigma[compared] > 0).mean())}
    for value in out.values():
        if isinstance(value, numpy.ndarray):
            value.setflags(write=False)
    return out
